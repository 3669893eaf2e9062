"""Without a GPU: every case of tests/test_ngu_curl_limits_gpu.py holds what it is named for, ngu_ref.knn_fast equals the
plain loop ngu_ref.knn, and its fold of the count past 2^30 changes neither the ring nor any later distance."""
import numpy as np
import pytest
import torch

import curl_ref as cr
import ngu_ref
from test_ngu_gpu import SHAPES, _head64, _three_rollouts

F32, F64 = np.float32, np.float64


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


# ---- the fast k-NN restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_knn_fast_equals_the_plain_loop_on_the_feature_tests_shapes(shape):
    n, t, m, k, e = shape
    slow = fast = (None, None, np.zeros((n, m, e), F32), np.zeros(n, np.int32))
    for emb, dones in _three_rollouts(shape):
        slow = ngu_ref.knn(emb, dones, slow[2], slow[3], k)
        fast = ngu_ref.knn_fast(emb, dones, fast[2], fast[3], k)
        assert all(_same(x, y) for x, y in zip(slow, fast))


def test_the_fold_keeps_the_ring_and_every_later_distance():
    case = ngu_ref.knn_limit_case("fold")
    n, t, m, k, e = case["shape"]
    assert m & (m - 1) and (case["ins0"] == [1 << 30, (1 << 30) + 3, (1 << 30) + 3]).all()
    assert case["calls"][0][1][2, 1] and not any(d[:2].any() for _, d in case["calls"])     # env 2 alone has a done
    folded = (None, None, case["mem0"], case["ins0"])
    plain = slow = (None, None, case["mem0"], case["ins0"].astype(np.int64))
    counts = []
    for emb, dones in case["calls"]:
        folded = ngu_ref.knn_fast(emb, dones, folded[2], folded[3], k)
        plain = ngu_ref.knn_fast(emb, dones, plain[2], plain[3], k, fold_counts=False)
        slow = ngu_ref.knn(emb, dones, slow[2], slow[3], k)
        assert all(_same(x, y) for x, y in zip(folded[:3], plain[:3])) and all(_same(x, y) for x, y in zip(plain, slow))
        assert ((plain[3] - folded[3]) % m == 0).all() and (folded[1].reshape(n, t)[:2] == k).all()   # the ring stays full
        counts.append(folded[3].tolist())
    # 2^30 itself is not folded (and becomes 2^30 + 4, which the next call folds); 2^30 + 3 is, at once; a done restarts
    assert counts == [[(1 << 30) + 4, 11, 3], [12, 15, 7], [16, 19, 11]]
    assert plain[3].tolist() == [(1 << 30) + 12, (1 << 30) + 15, 11]
    # a plain `mod M` would leave 1 + 4 = 5 < M entries: the next call's first row would find 5 candidates, not 6
    assert ((1 << 30) + 3) % m + t < m
    assert ngu_ref.fold(np.array([5, 1 << 30, (1 << 30) + 1], np.int32), 6).tolist() == [5, 1 << 30, 6 + ((1 << 30) + 1) % 6]


# ---- arl_epi_knn's cases ---------------------------------------------------------------------------------------------------

def test_knn_cases_hold_what_they_are_named_for():
    assert len(set(ngu_ref.KNN_LIMIT_NAMES)) == 8
    c = ngu_ref.knn_limit_case("scans")
    (e1, d1), (e2, d2) = c["calls"]
    assert c["shape"] == (2, 300, 8, 3, 4) and np.flatnonzero(d1[0]).tolist() == [70, 270] and not d1[1].any()
    assert 270 > 256 > 70 > 64 and 270 < 299 and not d2.any() and 300 - 8 > 270     # past both strides, not the last row
    c = ngu_ref.knn_limit_case("short-ring")
    n, t, m, k, e = c["shape"]
    assert (t, m) == (4096, 5) and sum(t0 >= m for t0 in range(0, t, 4)) == t // 4 - 2 and len(c["calls"]) == 2
    c = ngu_ref.knn_limit_case("long-ring")
    assert c["shape"] == (3, 9, 4096, 16, 128) and len(c["calls"]) == 3 and 3 * 9 < 4096 and c["calls"][1][1][1, 4]
    for name, width in (("width-28", 28), ("width-32", 32)):
        c = ngu_ref.knn_limit_case(name)
        assert c["shape"] == (2, 70, 130, 16, width) and width <= 32 and len(c["calls"]) == 3
        assert [int(np.flatnonzero(d[0])[0]) for _, d in c["calls"]] == [0, 35, 69] and not any(d[1].any() for _, d in c["calls"])
    c = ngu_ref.knn_limit_case("envs-65535")
    assert c["shape"] == (65535, 1, 1, 1, 4) and [int(d.sum()) for _, d in c["calls"]] == [0, 1, 0] and c["calls"][1][1][1234, 0]
    state = (None, None, c["mem0"], c["ins0"])
    for call, (emb, dones) in enumerate(c["calls"]):
        state = ngu_ref.knn_fast(emb, dones, state[2], state[3], 1)
        want_m = np.full(65535, int(call > 0), np.int32)
        want_m[1234] = 0 if call == 1 else want_m[1234]
        assert (state[1] == want_m).all() and _same(state[2][:, 0], emb[:, 0])         # the single slot: the newest row
        assert call != 1 or state[0][7, 0] == 0                                         # env 7 meets its own row again
    assert state[3].tolist().count(3) == 65534 and state[3][1234] == 2


def test_knn_4096_case_one_lane_holds_the_sixteen_nearest_and_twenty_lanes_hold_equal_ones():
    c = ngu_ref.knn_limit_case("full-4096")
    n, t, m, k, e = c["shape"]
    assert (n, t, m, k) == (1, 4096, 4096, 16) and not any(d.any() for _, d in c["calls"])
    first = ngu_ref.knn_fast(*c["calls"][0], c["mem0"], c["ins0"], k)
    assert first[3][0] == 4096 and (first[1] == np.minimum(np.arange(4096), 16)).all()   # the second call meets a full ring
    knn2, m2, _, ins = ngu_ref.knn_fast(*c["calls"][1], first[2], first[3], k)
    assert (m2 == 16).all() and ins[0] == 8192
    # every row of the second call has M = 4096 candidates, 64 per lane: ages 0 .. M - t - 1 staged from index 0, then
    # the rollout's rows from max(t0 - M, 0) = 0 on, so rollout row r passes through lane r mod 64
    q, nb = ngu_ref.LANE_ROW, ngu_ref.LANE_NEIGHBOURS
    assert len(nb) == 16 and max(nb) < q and len({r % 64 for r in nb}) == 1 and 4 * (q // 4) - m < 0
    assert knn2[q].tolist() == [(0.25 * (i + 1)) ** 2 for i in range(16)]                 # the planted ones ARE the nearest
    emb = c["calls"][1][0][0].astype(F64)
    others = np.setdiff1d(np.arange(q), nb)
    assert ((emb[others] - emb[q]) ** 2).sum(axis=1).min() > 16.0 and ((first[2][0].astype(F64) - emb[q]) ** 2).sum(1).min() > 16
    q, dup = ngu_ref.DUP_ROW, ngu_ref.DUP_ROWS
    assert len(dup) == 20 and max(dup) < q and len({r % 64 for r in dup}) == 20           # twenty lanes hold one each
    assert all(_same(c["calls"][1][0][0, r], c["calls"][1][0][0, q]) for r in dup) and not knn2[q].any() and m2[q] == 16


# ---- arl_epi_mix's cases ---------------------------------------------------------------------------------------------------

def test_mix_row_cases_reach_a_threads_second_and_third_row():
    assert ngu_ref.MIX_LIMIT_ROWS == (1024, 1025, 3000) and ngu_ref.MIX_LIMIT_K == (16, 1)
    for k in ngu_ref.MIX_LIMIT_K:
        for c in ngu_ref.mix_rows_case(1025, k, True):
            assert c["m"].min() == 0 and c["m"].max() == k and c["knn"].shape == (1025, k)
            valid = np.arange(k)[None, :] < c["m"][:, None]
            assert np.isfinite(c["knn"][valid]).all() and np.isinf(c["knn"][~valid]).all()
            assert (np.sort(c["knn"], axis=1) == c["knn"]).all()


def _planted(name, **over):
    c = ngu_ref.mix_planted_case(name)
    kw = dict(c_ext=c["c_ext"], c_int=c["c_int"], err=c["err"])
    kw.update(over)
    r_mix, dist, mom, diag = ngu_ref.mix(c["knn"], np.minimum(c["m"], c["k"]), kw["err"], c["r_ext"], c["dist0"], c["mom0"],
                                         c_ext=kw["c_ext"], c_int=kw["c_int"], **c["par"])
    return c, r_mix, dist, mom, diag


def test_mix_planted_cases_take_each_branch_in_some_row_and_not_in_another():
    c, r_mix, dist, _, diag = _planted("all-m-zero")
    assert not c["m"].any() and _same(dist, c["dist0"]) and dist[1] == 0.3 and diag[0] == 0
    assert _same(r_mix, (2.0 * c["r_ext"].astype(F64)).astype(F32))
    c, _, dist, _, _ = _planted("m-above-k")
    k, m = c["k"], c["m"]
    assert (m == k + 5).any() and (m == 2 ** 31 - 1).any() and (m <= k).any() and np.isfinite(c["knn"][m > k]).all()
    assert dist[0] == 7.0 + np.minimum(m, k).sum() != 7.0 + m.astype(F64).sum()
    c, r_mix, dist, _, _ = _planted("zero-distances", c_ext=0.0)
    assert not c["dist0"].any() and dist[1] == 0 and dist[0] > 0 and (r_mix > 0).all()   # 0 / 1e-8, not 0 / 0
    c, r_mix, dist, _, _ = _planted("tiny-distances", c_ext=0.0)
    assert 0 < dist[1] < 1e-8 and c["par"]["xi"] == 0
    by_mean = [1.0 / (np.sqrt(sum(1e-3 / (d / dist[1] + 1e-3) for d in row[:mj])) + 1e-3) for row, mj in zip(c["knn"], c["m"])]
    assert not np.allclose(r_mix, by_mean, rtol=0.1)                  # the mean as the divisor gives other rewards
    _, _, generic, _, _ = _planted("xi-large")
    assert generic[1] > 1e-8                                          # (and there the clamp is not taken)
    c, r_epi, _, _, _ = _planted("s-max-split", c_ext=0.0)
    zeros = (c["knn"] == 0).sum(axis=1)
    assert c["par"]["s_max"] == 2.0 and (c["m"] > 0).all() and (r_epi[zeros >= 4] == 0).all() and (zeros >= 4).any()
    assert (r_epi[zeros < 4] > 0).all() and (zeros < 4).any()
    c, _, _, mom, diag = _planted("modulator")
    alpha = 1.0 + (c["err"].astype(F64) - mom[1]) / np.sqrt(mom[2] / mom[0] + 1e-8)
    clip = c["par"]["mod_clip"]
    assert (alpha < 1).any() and ((alpha > 1) & (alpha < clip)).any() and (alpha > clip).any() and c["m"].size > 1024
    assert 1 < diag[1] < clip
    c, r_epi, dist, _, _ = _planted("xi-large", c_ext=0.0)
    finite = c["knn"][np.isfinite(c["knn"])]
    assert finite.max() / dist[1] < c["par"]["xi"]                    # every dn is 0: K = 1, s = sqrt(m) + c
    assert np.allclose(r_epi, 1.0 / (np.sqrt(c["m"]) + c["par"]["c"]), rtol=1e-6)
    c, _, dist, _, _ = _planted("m-above-k")
    assert (finite.max() > 0) and (c["knn"][np.isfinite(c["knn"])] / dist[1] > c["par"]["xi"]).any()   # and elsewhere not


# ---- arl_invdyn_loss_parts' cases ------------------------------------------------------------------------------------------

def test_invdyn_lds_boundary_from_the_layout_and_from_the_library(lib):
    a_max = ngu_ref.invdyn_a_max(32, 256)
    assert a_max == 13
    assert 4 * ngu_ref.invdyn_lds_floats(32, 256, a_max) <= 159 * 1024 < 4 * ngu_ref.invdyn_lds_floats(32, 256, a_max + 1)
    assert lib.arl_invdyn_workspace_bytes(32, 256, a_max) > 0 and lib.arl_invdyn_workspace_bytes(32, 256, a_max + 1) == 0
    for width, hidden in ((4, 4), (20, 36), (128, 64), (32, 128)):    # every other size of the GPU file: all 64 actions fit
        assert ngu_ref.invdyn_a_max(width, hidden) == 64 and lib.arl_invdyn_workspace_bytes(width, hidden, 64) > 0
    # the two corners of ceil(2 width / 32) ceil(hidden / 32) <= 16, and one step past each
    blocks = lambda width, hidden: -(-2 * width // 32) * -(-hidden // 32)                 # noqa: E731
    assert blocks(128, 64) == blocks(32, 256) == 16 and blocks(128, 68) > 16 and blocks(36, 256) > 16
    assert lib.arl_invdyn_workspace_bytes(128, 68, 2) == 0 and lib.arl_invdyn_workspace_bytes(36, 256, 2) == 0
    assert (2 * 20) % 32 and 36 % 32 and (33 | 1) == 33 and (64 | 1) == 65 and (32 | 1) == 33


def _head_loss(host, actions, weight, n_act):
    leaves = [torch.from_numpy(a.astype(F32)).double() for a in host]
    return _head64(*leaves, torch.from_numpy(np.minimum(actions.astype(np.int64), n_act - 1)), torch.from_numpy(weight))


def test_invdyn_edge_inputs_hold_what_they_are_named_for():
    sizes = (4, 4, 33)
    host, actions, weight = ngu_ref.invdyn_case(65, sizes, weights="sum0.3")
    assert abs(weight.sum() - 0.3) < 1e-6 and (weight > 0).all()
    loss, acc = _head_loss(host, actions, weight, 33)
    loss1, acc1 = _head_loss(host, actions, weight / weight.sum(), 33)
    assert abs(loss.item() - weight.sum() * loss1.item()) < 1e-12 and abs(acc.item() - weight.sum() * acc1.item()) < 1e-12
    _, _, weight = ngu_ref.invdyn_case(65, sizes, weights="sum1.7")
    assert abs(weight.sum() - 1.7) < 1e-6
    host, actions, weight = ngu_ref.invdyn_case(65, sizes, over=True)
    assert (actions == 255).any() and (actions == 33).any() and (actions < 33).any() and weight[actions >= 33].any()
    _, _, weight = ngu_ref.invdyn_case(65, sizes, weights="last-only")
    assert np.flatnonzero(weight).tolist() == [64]
    for b, s in ((2049, (4, 4, 2)), (4097, (4, 4, 2)), (2049, (32, 128, 18))):
        host, actions, weight = ngu_ref.invdyn_case(b, s, ones_from=2048)
        top = np.sort(ngu_ref.invdyn_logits64(host, b), axis=1)
        assert (top[:, -1] - top[:, -2]).min() > 1e-4 and (weight[2048:] == 1).all() and 0 < weight[:2048].sum() < 2048
        assert -(-b // 32) > 64 * ((b - 1) // 2048)                   # 65 tiles: a second trip; 129: a third


# ---- arl_curl_loss_parts' cases --------------------------------------------------------------------------------------------

def _deal_out(d):
    """the reduction over D in S: wave w adds k in [kb, ke) -- kq = (D / 4 + 1) & ~1"""
    kq = (d // 4 + 1) & ~1
    return [(w * kq, min(w * kq + kq, d)) for w in range(4)]


def test_curl_widths_reach_every_deal_out_and_block_count():
    empty = lambda d: [w for w, (kb, ke) in enumerate(_deal_out(d)) if kb >= ke]          # noqa: E731
    for d in (4, 8, 12, 32, 36, 64, 68, 100, 124, 128):
        spans = [(kb, ke) for kb, ke in _deal_out(d) if kb < ke]
        assert spans[0][0] == 0 and spans[-1][1] == d and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert empty(8) == [] and empty(12) == [3] and empty(4) == [2, 3]                     # a quarter that adds nothing
    assert _deal_out(100)[3] == (78, 100) and _deal_out(124)[3] == (96, 124)              # a last quarter shorter than kq
    blocks = lambda d: -(-d // 32)                                                        # noqa: E731
    assert blocks(32) == 1 and blocks(64) == 2 and blocks(68) == 3 and blocks(100) == 4 and 100 % 32 and 68 % 32 == 4
    assert blocks(68) ** 2 == 9 and [q for q in range(9) if q % 4 == 0] == [0, 4, 8]      # wave 0 owns a third dW block


@pytest.mark.parametrize("b,d", [(2048, 4), (2049, 4), (4096, 4), (2049, 128), (4096, 128), (33, 8), (65, 12), (33, 68),
                                 (65, 100), (65, 124), (65, 36)])
def test_curl_random_cases_decide_every_arg_max(b, d):
    zq, zk, w, s = cr.random_case(b, d)
    assert cr.margins(s).min() > cr.MARGIN and 0.5 < np.abs(s).max() < 100
    assert np.allclose(s, cr.logits64(zq, zk, w), rtol=0, atol=1e-9) and 0 < cr.hits(s) < b
    assert -(-b // 32) > 64 or b <= 2048                              # past 2048 rows a workgroup takes a second tile


@pytest.mark.parametrize("b,d", [(65, 36), (2049, 36)])
def test_curl_planted_rows(b, d):
    zq, zk, w, s = cr.planted_case(b, d)
    a, last = cr.PLANTED_ROW, b - 1
    assert cr.margins(s).min() > cr.MARGIN
    before = s[a, :32 * (last // 32)]                                 # every key of an earlier key tile
    assert s[a].argmax() == last and last // 32 > before.argmax() // 32 and s[a, last] - before.max() > 100
    assert s[a, last] - np.delete(s[a], last).max() > 1 and np.exp(F32(before.max() - s[a, last])) == 0
    assert s[a, last] - s[a, a] > 100                                 # that row's loss: dropping the last tile moves it by O(100)
    assert b % 32 == 1 and last // 32 == b // 32 and s[last].argmax() == last            # ragged tile, diagonal in the last key tile
    assert s[last, last] - np.delete(s[last], last).max() > 1


def test_curl_ties_are_exact_and_everything_else_is_decided():
    b, d = 65, 36
    zq, zk, w, s = cr.tie_case(b, d)
    assert sum(r < p for r, p in cr.TIES) == 3 and sum(r > p for r, p in cr.TIES) == 1
    assert {r // 32 == p // 32 for r, p in cr.TIES} == {True, False}  # inside one key tile, and across
    p64 = zq.astype(F64) @ w.astype(F64)
    rest = np.ones(b, bool)
    rest[[p for _, p in cr.TIES]] = False
    for r, p in cr.TIES:
        assert _same(zk[r], zk[p])
        # equal keys give equal logits under any fixed order of the sum over D: here e ascending, in float64 and in fp32
        for dtype in (F64, F32):
            pr, acc = p64[r].astype(dtype), [dtype(0), dtype(0)]
            for e in range(d):
                acc = [acc[0] + pr[e] * dtype(zk[r, e]), acc[1] + pr[e] * dtype(zk[p, e])]
            assert acc[0] == acc[1]
        assert s[r, r] == s[r, p] == s[r].max() and s[r, r] - s[r, rest & (np.arange(b) != r)].max() > 1
        assert s[p].max() > s[p, r] + cr.MARGIN                       # row p's own maximum lies elsewhere
    others = np.setdiff1d(np.arange(b), [r for r, _ in cr.TIES])
    assert cr.margins(s[others][:, rest]).min() > cr.MARGIN
    first = cr.hits(s)
    last = int((b - 1 - np.argmax(s[:, ::-1], axis=1) == np.arange(b)).sum())
    assert first - last == 2                                          # `>=` in the arg-max scan: three hits become one
