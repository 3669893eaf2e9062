"""The LayerNorm, pooling and return-scan kernels at the limits their entry points accept (csrc/layernorm.hip,
csrc/qlambda_scan.hip, csrc/vtrace_scan.hip, the Retrace scan of csrc/acer.hip, csrc/resnet.hip).  The feature tests
(test_pqn_gpu.py, test_vtrace_gpu.py, test_acer_gpu.py, test_resnet_gpu.py) stay as they are; this file runs the shapes
they leave out:

- LayerNorm: widths just past every dispatch boundary and with dead or half-dead float4 slots (8, 36, 68, 256, 260, 516,
  768, 1020), the forward's second (ragged) trip over 2048 blocks at every LPR, both backward variants, dz over dy and
  elsewhere, every output inside a NaN-filled buffer -- and y, stats, dz and the per-block partial rows held BIT FOR BIT
  to the fp32 restatement of the header's lane layout and summation order (tests/ln_ref.py), dgamma / dbeta to those
  partials folded by noisy_ref.fold_f32; the first-order bounds of DESIGN.md 22 are asserted alongside;
- the Q(lambda) scan at horizons round the lane wrap up to the limit of 4096 (36 KiB of LDS), action counts that leave
  one to three entries of the last float4 live, the action and stride limits, a block index above 65535;
- the V-trace and the Retrace scan at horizons with a ragged first chunk, dones and clipped ratios planted on both sides
  of every chunk edge, a block index above 65535;
- the residual network's four grid-stride kernels past the wrap at 2048 x 256 threads, and at the channel limit.

Out of scope: the 64-bit branch of split_index and rows * width >= 2^31 need buffers of tens of GiB; pooling windows made
entirely of -inf or NaN are not part of any contract the header states."""
import numpy as np
import pytest
import torch

import acer_ref as ar
import ln_ref as lr
import pqn_ref as pr
import resnet_ref as rr
import vtrace_ref as vr
from ln_ref import EPS, LN_ROWS, LN_SECOND_TRIP, LN_WIDTHS
from test_acer_gpu import _scan as rt_scan
from test_pqn_gpu import _scan_case as ql_case
from test_resnet_host import pool_input
from test_vtrace_gpu import KEYS, _launch as vt_launch, _on_device as vt_on_device, _scan_case as vt_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
PAD = 64                                                        # guard floats behind every output
WRAP = 2048 * 256                                               # the grid-stride walks of csrc/resnet.hip wrap from here


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _guarded(shape, fill=NAN, dtype=torch.float32, pad=PAD):
    """-> (the whole buffer, its leading view of `shape`): the view is what a kernel is given."""
    n = int(np.prod(shape))
    big = torch.full((n + pad,), fill, dtype=dtype, device=DEV)
    return big, big[:n].view(shape)


def _tail_untouched(big, n, fill=NAN):
    tail = big[n:]
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def _same_bits(got, want, what):
    got, want = _host(got) if torch.is_tensor(got) else got, np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(lr.bits(got), lr.bits(want), err_msg=str(what))


# ---- LayerNorm + rectifier ---------------------------------------------------------------------------------------------

def _ln_forward(L, z_d, gamma_d, beta_d):
    rows, width = z_d.shape
    y_big, y = _guarded((rows, width))
    st_big, stats = _guarded((rows, 2))
    L.ln_relu_fwd(z_d, gamma_d, beta_d, EPS, y, stats)
    torch.cuda.synchronize()
    assert _tail_untouched(y_big, rows * width) and _tail_untouched(st_big, 2 * rows)
    return y, stats


def _ln_backward(L, dy, y, z_d, stats, gamma_d, masked, in_place, deferred=False):
    """-> (dz, dgamma, dbeta, part_g, part_b) on the host, after the guards round every output have been checked."""
    rows, width = dy.shape
    grid = pr.ln_shape(rows, width)[2]
    dy_big, dy_d = _guarded((rows, width))
    dy_d.copy_(_dev(dy))
    dz_big, dz = (dy_big, dy_d) if in_place else _guarded((rows, width))
    dg_big, dg = _guarded((width,))
    db_big, db = _guarded((width,))
    ws_floats = L.ln_bwd_workspace(DEV).numel()
    ws_big, ws = _guarded((ws_floats,))
    if deferred:
        folds = L.FoldList()
        folds.ln_relu_bwd(dy_d, y, z_d, stats, gamma_d, masked, dz, dg, db, ws)
        torch.cuda.synchronize()
        assert torch.isnan(dg).all() and torch.isnan(db).all()                  # nothing folded before run()
        folds.run()
    else:
        L.ln_relu_bwd(dy_d, y, z_d, stats, gamma_d, masked, dz, dg, db, ws)
    torch.cuda.synchronize()
    used = 2 * grid * width
    assert _tail_untouched(dz_big, rows * width) and _tail_untouched(dg_big, width) and _tail_untouched(db_big, width)
    assert _tail_untouched(ws_big, used), "the workspace past 2 * grid * width floats"
    assert torch.isfinite(ws_big[:used]).all()
    if not in_place:
        _same_bits(dy_d, dy, "dy is an input")
    part = _host(ws[:used]).reshape(2, grid, width)             # part_g at offset 0, part_b at grid * width floats
    return _host(dz), _host(dg), _host(db), part[0], part[1]


def _ln_check(L, rows, width, variants):
    """One case: the forward and every (dy_masked, in_place) of `variants` against the fp32 restatement bit for bit and
    against float64 within the bound -> the error / bound ratios."""
    z, gamma, beta, dy = lr.ln_case(rows, width)
    z_d, gamma_d, beta_d = _dev(z), _dev(gamma), _dev(beta)
    y, stats = _ln_forward(L, z_d, gamma_d, beta_d)
    want_y, want_stats = lr.ln_relu_fwd32(z, gamma, beta, EPS)
    tag = (rows, width)
    _same_bits(stats[:, 0], want_stats[:, 0], ("mean",) + tag)
    _same_bits(stats[:, 1], want_stats[:, 1], ("rstd",) + tag)
    _same_bits(y, want_y, ("y",) + tag)
    yh, sh = _host(y), _host(stats)
    mask = yh > 0
    assert mask.any() and not mask.all()
    y64, mean64, rstd64 = pr.ln_relu_fwd64(z, gamma, beta, EPS)
    e_y, e_mean, e_rstd = pr.ln_fwd_bound(z, gamma, beta, EPS)
    ratios = dict(y=(np.abs(yh - y64) / e_y).max(), mean=(np.abs(sh[:, 0] - mean64) / e_mean).max(),
                  rstd=(np.abs(sh[:, 1] - rstd64) / e_rstd).max())
    dz64, dg64, db64 = pr.ln_relu_bwd64(dy, mask, z, gamma, EPS)
    e_dz, e_dg, e_db = pr.ln_bwd_bound(dy, mask, z, gamma, EPS)
    dy_premasked = np.where(mask, dy, np.float32(0))
    for masked, in_place in variants:
        dy_in = dy_premasked if masked else dy
        got = _ln_backward(L, dy_in, y, z_d, stats, gamma_d, masked, in_place)
        want_dz, want_pg, want_pb = lr.ln_relu_bwd32(dy_in, None if masked else yh, z, sh, gamma, masked)
        var = tag + (masked, in_place)
        _same_bits(got[0], want_dz, ("dz",) + var)
        _same_bits(got[3], want_pg, ("part_g",) + var)
        _same_bits(got[4], want_pb, ("part_b",) + var)
        _same_bits(got[1], lr.ln_fold32(want_pg), ("dgamma",) + var)
        _same_bits(got[2], lr.ln_fold32(want_pb), ("dbeta",) + var)
        ratios.update(dz=(np.abs(got[0] - dz64) / np.maximum(e_dz, 1e-300)).max(),
                      dgamma=(np.abs(got[1] - dg64) / np.maximum(e_dg, 1e-300)).max(),
                      dbeta=(np.abs(got[2] - db64) / np.maximum(e_db, 1e-300)).max())
        for k, v in ratios.items():
            assert v <= 1.0, (k, v) + var
    # the backward pass leaves its inputs alone
    for t, a, what in ((z_d, z, "z"), (gamma_d, gamma, "gamma"), (beta_d, beta, "beta"), (y, yh, "y"), (stats, sh, "stats")):
        _same_bits(t, a, what)
    print("ln rows %5d width %4d error / bound: %s" % (rows, width, " ".join("%s %.3f" % kv for kv in ratios.items())))
    return ratios


ALL_VARIANTS = ((0, False), (0, True), (1, False), (1, True))


@pytest.mark.parametrize("width", LN_WIDTHS)
def test_ln_equals_the_fp32_restatement_bit_for_bit_at_every_dispatch_edge(L, width):
    """Widths just past every <LPR, V> boundary, with half-dead butterflies (36: 9 of 16 lanes, 68: 17 of 64) and float4
    slots partly or wholly dead (260: one live lane in v = 1; 516: one in v = 2, none in v = 3; 768: none in v = 3; 1020:
    the last lane of v = 3 dead), at rows 1, 3, 65 and 1031.  Largest error / bound per width on an MI355X: DESIGN.md 22."""
    worst = {}
    for rows in LN_ROWS:
        for k, v in _ln_check(L, rows, width, ALL_VARIANTS).items():
            worst[k] = max(worst.get(k, 0.), v)
    print("ln width %4d largest error / bound: %s" % (width, " ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("rows,width", LN_SECOND_TRIP, ids=lambda v: str(v))
def test_ln_forward_second_trip_with_a_ragged_tail(L, rows, width):
    """More than 2048 * RPB rows: the forward's it = 1 trip runs, its last block half empty; the backward takes nine
    trips of 256 blocks."""
    grid, iters = lr.ln_fwd_grid(rows, width)
    assert (grid, iters) == (2048, 2)
    assert pr.ln_shape(rows, width)[2:4] == (256, 9)
    _ln_check(L, rows, width, ((0, False), (1, True)))


@pytest.mark.parametrize("rows,width", [(1031, 100), (1031, 1024)])
def test_ln_deferred_fold_gives_the_bits_of_the_immediate_one(L, rows, width):
    """FoldList.ln_relu_bwd + run() against ln_relu_bwd; at (1031, 1024) the grid is 256 and the workspace is used to its
    last float (the guard behind it stays NaN)."""
    z, gamma, beta, dy = lr.ln_case(rows, width)
    if width == 1024:
        assert 2 * pr.ln_shape(rows, width)[2] * width == L.ln_bwd_workspace(DEV).numel()
    y, stats = _ln_forward(L, _dev(z), _dev(gamma), _dev(beta))
    now = _ln_backward(L, dy, y, _dev(z), stats, _dev(gamma), 0, False)
    later = _ln_backward(L, dy, y, _dev(z), stats, _dev(gamma), 0, False, deferred=True)
    for a, b, what in zip(now, later, ("dz", "dgamma", "dbeta", "part_g", "part_b")):
        _same_bits(a, b, what)
    _same_bits(now[1], lr.ln_fold32(now[3]), "dgamma")
    _same_bits(now[2], lr.ln_fold32(now[4]), "dbeta")
    want = lr.ln_relu_bwd32(dy, _host(y), z, _host(stats), gamma, 0)
    for a, b, what in zip((now[0], now[3], now[4]), want, ("dz", "part_g", "part_b")):
        _same_bits(a, b, what)


# ---- Q(lambda) scan ----------------------------------------------------------------------------------------------------

def _ql_inputs(n_env, horizon, n_act, stride, seed):
    """test_pqn_gpu._scan_case (dones at the first step, at the last step, on consecutive steps) with +inf in the padding
    columns (a NaN would be swallowed by fmaxf) and dones at t = 63 and t = 64, the lane wrap."""
    q, q_last, r, d = ql_case(n_env, horizon, n_act, seed, stride=stride)
    q[:, :, n_act:] = INF
    q_last[:, n_act:] = INF
    for t in (63, 64):
        if t < horizon:
            d[t % n_env, t] = 1
    if horizon > 64:
        d[:, 60:63] = 0                                         # (so that a return really crosses into t = 63)
    return q, q_last, r, d


def _ql_check(L, n_env, horizon, n_act, stride, lams=(0.0, 0.65, 1.0), discounts=(0.99,), seed=0, no_dones=False):
    q, q_last, r, d = _ql_inputs(n_env, horizon, n_act, stride, seed + n_env + horizon + n_act + stride)
    if no_dones:
        d[:] = 0
    assert (d == 0).any()                                       # some step reads its bootstrap row
    dev = [_dev(q.reshape(-1, stride)), _dev(q_last), _dev(r.reshape(-1)), _dev(d.reshape(-1))]
    for discount in discounts:
        for lam in lams:
            big, out = _guarded((n_env * horizon,))
            L.qlambda_scan(dev[0], dev[1], dev[2], dev[3], discount, lam, n_env, horizon, n_act, out)
            torch.cuda.synchronize()
            want = pr.qlambda_scan64(q, q_last, n_act, r, d, discount, lam)
            assert np.isfinite(want).all()
            _same_bits(_host(out).reshape(n_env, horizon), want, (n_env, horizon, n_act, stride, discount, lam))
            assert _tail_untouched(big, n_env * horizon)
    for t, a in zip(dev, (q.reshape(-1, stride), q_last, r.reshape(-1), d.reshape(-1))):
        np.testing.assert_array_equal(_host(t), a)              # the inputs are left alone


@pytest.mark.parametrize("horizon", [63, 64, 65, 129, 1024, 4095, 4096])
def test_qlambda_scan_at_the_lane_wrap_and_the_horizon_limit(L, horizon):
    """4096 steps take 36 KiB of dynamic LDS; discount 1.0 runs once, there."""
    _ql_check(L, 2, horizon, 6, 32, discounts=(0.99, 1.0) if horizon == 4096 else (0.99,))


@pytest.mark.parametrize("n_act,stride", [(1, 4), (2, 4), (3, 4), (5, 8), (7, 8), (63, 64), (64, 64), (64, 68)])
def test_qlambda_scan_action_counts_and_strides(L, n_act, stride):
    """One to three live entries in the last float4, the action limit, a stride beyond it; +inf in every padding column."""
    _ql_check(L, 2, 65, n_act, stride)


def test_qlambda_scan_at_the_stride_limit(L):
    """q_stride = 2^20: 8 MB of q rows and 4 MB of q_last for two steps of one env (no dones: the plants of a longer
    rollout would end both steps, and neither row maximum would be read)."""
    _ql_check(L, 1, 2, 64, 2 ** 20, no_dones=True)


def test_qlambda_scan_block_index_above_65535(L):
    _ql_check(L, 70001, 1, 6, 8)


# ---- V-trace scan ------------------------------------------------------------------------------------------------------

CHUNK = 1024                    # VT_CHUNK of csrc/vtrace_scan.hip and AC_CHUNK of csrc/acer.hip: change it with them


def _chunk_edges(horizon):
    """The walk comes from the end: step k closes a chunk, step k - 1 opens the next, k = T - 1024, T - 2048, .."""
    return list(range(horizon - CHUNK, 0, -CHUNK))


def _vt_inputs(horizon, n_act):
    """test_vtrace_gpu._scan_case for two envs, and on both sides of every chunk edge k (_chunk_edges): a done at k - 1
    in env 0, a done at k in env 1, and in env 1 a ratio of 8 (above every rho_bar used) at k - 1 and at k."""
    c = vt_case(2, horizon, n_act)
    edges = _chunk_edges(horizon)
    for k in edges:
        c["dones"][0, k - 1] = 1
        c["dones"][0, k] = 0
        c["dones"][1, k] = 1
        c["dones"][1, k - 1] = 0
        for t in (k - 1, k):
            a = min(int(c["actions"][1, t]), n_act - 1)
            c["prob"][1, t, a] = max(c["prob"][1, t, a], np.float32(1e-3))
            c["old_prob"][1, t, a] = c["prob"][1, t, a] / np.float32(8)
    return c, edges


@pytest.mark.parametrize("horizon,n_act", [(1023, 18), (1024, 18), (1025, 18), (2049, 18), (4095, 18), (1025, 1)])
def test_vtrace_scan_across_ragged_chunks_and_planted_edges(L, horizon, n_act):
    """T % 1024 != 0 leaves a ragged chunk at lo = 0; acc_next, vs_next, v_next, ratio_sum and n_clipped cross every edge
    with a done on either side of it."""
    c, edges = _vt_inputs(horizon, n_act)
    assert len(edges) == (horizon - 1) // CHUNK
    dc = vt_on_device(c)
    ratio = vr.ratios64(c["prob"], c["old_prob"], c["actions"])
    for k in edges:
        assert ratio[1, k - 1] > 2.0 and ratio[1, k] > 2.0 and c["dones"][0, k - 1] and c["dones"][1, k]
    for lam in (0.0, 0.95, 1.0):
        for bars in ((1.0, 1.0, 1.0), (2.0, 0.5, 1.0)):
            got = vt_launch(L, c, dc, lam, bars)
            vs, adv, stats = vr.vtrace_walk(ratio, c["values"], c["last_values"], c["rewards"], c["dones"], 0.99, lam, *bars)
            assert stats[1, 1] >= 2 * len(edges)
            msg = (horizon, n_act, lam, bars)
            _same_bits(got[0], vs.astype(np.float32), ("returns",) + msg)
            _same_bits(got[1], adv.astype(np.float32), ("advantages",) + msg)
            _same_bits(got[2], stats, ("stats",) + msg)
    for k in KEYS:
        np.testing.assert_array_equal(_host(dc[k]).reshape(c[k].shape), c[k])              # the inputs are left alone
    if horizon == 2049:                                         # determinism: a second launch, the same bits
        first, again = vt_launch(L, c, dc, 0.95, (2.0, 0.5, 1.0)), vt_launch(L, c, dc, 0.95, (2.0, 0.5, 1.0))
        for a, b in zip(first, again):
            _same_bits(a, b, "two launches")


def test_vtrace_scan_block_index_above_65535(L):
    n_env = 70001
    c = vr.rollout(7, n_env, 1, 6)
    c["dones"][::3] = 1
    dc = vt_on_device(c)
    ratio = vr.ratios64(c["prob"], c["old_prob"], c["actions"])
    for lam in (0.0, 0.95, 1.0):
        for bars in ((1.0, 1.0, 1.0), (2.0, 0.5, 1.0)):
            got = vt_launch(L, c, dc, lam, bars)
            vs, adv, stats = vr.vtrace_walk(ratio, c["values"], c["last_values"], c["rewards"], c["dones"], 0.99, lam, *bars)
            _same_bits(got[0], vs.astype(np.float32), "returns")
            _same_bits(got[1], adv.astype(np.float32), "advantages")
            _same_bits(got[2], stats, "stats")


# ---- Retrace scan ------------------------------------------------------------------------------------------------------

def _rt_want(c, lam):
    return ar.retrace(c["prob"], c["prob_last"], c["q"], c["q_last"], c["old_prob"], c["actions"], c["rewards"],
                      c["dones"], 0.99, lam, c["n_env"], c["horizon"])


def _rt_same(got, want, what):
    for g, w, name in zip(got, want, ("qret", "v", "stats")):
        _same_bits(g, w, (name,) + what)


@pytest.mark.parametrize("horizon,n_act", [(1023, 18), (1025, 18), (2049, 18), (1025, 1)])
def test_retrace_scan_across_ragged_chunks_and_planted_edges(L, horizon, n_act):
    """acer_ref.scan_case for two envs (action bytes of 255 among them), and on both sides of every chunk edge k: a done
    at k - 1 in env 0, a done at k in env 1, and in env 1 a rho of about 8 at k - 1 and at k, so that qret, rho_sum and
    n_above cross every edge with a done on either side of it."""
    c = ar.scan_case(horizon + n_act, 2, horizon, n_act, 64, act255=True)
    edges = _chunk_edges(horizon)
    assert len(edges) == (horizon - 1) // CHUNK
    dones, acts = c["dones"].reshape(2, horizon), c["actions"].reshape(2, horizon)
    prob, old = c["prob"].reshape(2, horizon, n_act), c["old_prob"].reshape(2, horizon, n_act)
    for k in edges:
        dones[0, k - 1], dones[0, k], dones[1, k - 1], dones[1, k] = 1, 0, 0, 1
        for t in (k - 1, k):
            a = min(int(acts[1, t]), n_act - 1)
            assert prob[1, t, a] >= 1e-3
            old[1, t, a] = prob[1, t, a] / np.float32(8)
    for lam in (0.0, 0.95, 1.0):
        want = _rt_want(c, lam)
        assert np.isfinite(want[0]).all() and want[2][1, 1] >= 2 * len(edges)
        _rt_same(rt_scan(L, c, lam), want, (horizon, n_act, lam))
    if horizon == 2049:                                         # determinism: a second launch, the same bits
        _rt_same(rt_scan(L, c, 0.95), rt_scan(L, c, 0.95), ("two launches",))


def test_retrace_scan_block_index_above_65535(L):
    c = ar.scan_case(11, 70001, 1, 6, 8, mu_zero=True, act255=True)
    c["dones"][::3] = 1
    for lam in (0.0, 1.0):
        _rt_same(rt_scan(L, c, lam), _rt_want(c, lam), (70001, lam))


# ---- the residual network's streaming kernels --------------------------------------------------------------------------

def test_add_relu_past_the_grid_stride_wrap(L):
    n = 4 * (WRAP + 259)
    assert n // 4 > WRAP
    rs = np.random.RandomState(n % 9973)
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    b[::7] = -a[::7]                                            # exact zeros among the sums
    want_s, want_r = rr.add_relu32(a, b)
    for alias in (None, "a", "b"):
        for with_relu in (True, False):
            runs = []
            for _ in range(2):                                  # twice: the same bits
                (a_big, ad), (b_big, bd) = _guarded((n,)), _guarded((n,))
                ad.copy_(_dev(a)), bd.copy_(_dev(b))
                out_big, out = dict(a=(a_big, ad), b=(b_big, bd)).get(alias) or _guarded((n,))
                relu_big, relu = _guarded((n,)) if with_relu else (None, None)
                L.add_relu(ad, bd, out, relu)
                torch.cuda.synchronize()
                _same_bits(out, want_s, (alias, with_relu))
                assert all(_tail_untouched(t, n) for t in (a_big, b_big, out_big))
                if with_relu:
                    _same_bits(relu, want_r, (alias, with_relu, "relu"))
                    assert _tail_untouched(relu_big, n)
                if alias != "a":
                    _same_bits(ad, a, "a is an input")
                if alias != "b":
                    _same_bits(bd, b, "b is an input")
                runs.append((out, relu))
            assert torch.equal(runs[0][0], runs[1][0]) and (not with_relu or torch.equal(runs[0][1], runs[1][1]))


def _pool_fwd(L, z_d, shape_out, with_relu, with_arg):
    n = int(np.prod(shape_out))
    y_big, y = _guarded(shape_out)
    r_big, y_relu = _guarded(shape_out) if with_relu else (None, None)
    a_big, arg = _guarded(shape_out, fill=255, dtype=torch.uint8) if with_arg else (None, None)
    L.maxpool3s2_fwd(z_d, y, y_relu, arg)
    torch.cuda.synchronize()
    assert _tail_untouched(y_big, n) and (r_big is None or _tail_untouched(r_big, n))
    assert a_big is None or _tail_untouched(a_big, n, fill=255)
    return y, y_relu, arg


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "floats"])
@pytest.mark.parametrize("shape", [(9, 33, 31, 1024), (1, 1, 2, 1024), (1, 2, 1, 4)], ids=lambda s: "x".join(map(str, s)))
def test_pool_past_the_grid_stride_wrap_and_at_the_channel_limit(L, shape, ties):
    """(9, 33, 31, 1024): 626 688 output and 2.36 M input float4s, so the forward's and the backward's walks both wrap;
    the channel limit, odd sides.  (1, 1, 2, 1024) and (1, 2, 1, 4): the degenerate sides at both channel ends."""
    b, h, w, c = shape
    oh, ow = rr.out_hw(h, w)
    shape_out = (b, oh, ow, c)
    if b > 1:
        assert b * oh * ow * (c // 4) > WRAP and b * h * w * (c // 4) > WRAP
    z = pool_input(shape, ties)
    dy = pool_input(shape_out, ties, seed=1)
    want_y, want_relu, want_arg = rr.maxpool_fwd32(z)
    want_dz = rr.maxpool_bwd32(dy, want_arg, h, w)
    z_d, dy_d, arg_d = _dev(z), _dev(dy), _dev(want_arg)
    runs = []
    for _ in range(2):
        y, y_relu, arg = _pool_fwd(L, z_d, shape_out, True, True)
        _same_bits(y, want_y, "y"), _same_bits(y_relu, want_relu, "y_relu")
        np.testing.assert_array_equal(_host(arg), want_arg)
        dz_big, dz = _guarded(shape)
        L.maxpool3s2_bwd(dy_d, arg_d, dz)
        torch.cuda.synchronize()
        _same_bits(dz, want_dz, "dz")
        assert _tail_untouched(dz_big, int(np.prod(shape)))
        runs.append((y, y_relu, arg, dz))
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    for with_relu, with_arg in ((False, False), (True, False), (False, True)):             # the optional outputs left out
        y, y_relu, arg = _pool_fwd(L, z_d, shape_out, with_relu, with_arg)
        assert torch.equal(y, runs[0][0])
        assert y_relu is None or torch.equal(y_relu, runs[0][1])
        assert arg is None or torch.equal(arg, runs[0][2])
    _same_bits(z_d, z, "z is an input"), _same_bits(dy_d, dy, "dy is an input")


@pytest.mark.parametrize("n,c,h,w", [(3, 5, 300, 300), (1, 1024, 3, 3)])
def test_gather_of_any_plane_past_the_wrap_and_at_the_channel_limit(L, n, c, h, w):
    """(3, 5, 300, 300): 540 000 float4s, the last channel group three-quarters padding.  (1, 1024, 3, 3): the limit."""
    rs = np.random.RandomState(n + c + h + w)
    obs = rs.randint(0, 256, size=(n, c, h, w), dtype=np.uint8)
    obs_d = _dev(obs)
    scale = np.float32(1. / 255)
    cp = (c + 3) // 4 * 4
    if n > 1:
        assert n * h * w * (cp // 4) > WRAP
    for idx in (None, rs.randint(0, n, size=n).astype(np.int32)):
        rows = np.arange(n) if idx is None else idx
        want = np.zeros((len(rows), h, w, cp), np.float32)
        want[..., :c] = obs[rows].transpose(0, 2, 3, 1).astype(np.float32) * scale
        runs = []
        for _ in range(2):
            big, out = _guarded(want.shape)
            L.gather_scale_obs_nhwc_any(obs_d, _dev(idx), out, float(scale))
            torch.cuda.synchronize()
            _same_bits(out, want, (n, c, h, w, idx is None))
            assert _tail_untouched(big, want.size)
            runs.append(out)
        assert torch.equal(*runs)
    np.testing.assert_array_equal(_host(obs_d), obs)
