"""The CPU-side twin of tests/test_batch_limits_gpu.py: on the very inputs of the device file (tests/batch_ref.py) it
shows that the case table reaches every scan route, that the references hold what the device file relies on, and that
each nearest wrong version of a kernel gives another answer -- so the device comparisons cannot pass by accident."""
import numpy as np
import pytest

import batch_ref as R
from batch_ref import F32, F64
from oracle import ref_port as P


# ---------------------------------------------------------------------------------------------------- scans

def test_case_table_reaches_every_route_for_both_alignments():
    for route, n, T in R.SCAN_CASES:
        assert R.scan_route(n, T, True) == route, (route, n, T)
        assert R.scan_route(n, T, False) == "direct", (n, T)          # without vec_ok there is one kernel
    assert set(c[0] for c in R.SCAN_CASES) == set(R.ROUTES)
    assert [R.SCAN_CASES[i][0] for i in R.SCAN_SUB] == list(R.ROUTES)
    # both thresholds of the tile rule, from either side
    assert R.scan_route(65408, 9, True) == "lds64" and R.scan_route(65409, 9, True) == "lds128"
    assert R.scan_route(130816, 8, True) == "lds128" and R.scan_route(130817, 8, True) == "lds256"
    # every other threshold of dispatch()
    assert [R.scan_route(70, T, True) for T in (17, 18, 34, 35, 36, 136, 137, 140, 544, 545, 548)] == \
        ["lds64", "lds64x256", "lds64x256", "lds32", "chunked", "chunked", "lds8", "chunked", "chunked", "direct", "chunked"]
    # the shapes the table is there for
    assert any(T % 64 and T > 64 and n > 64 and n % 32 for r, n, T in R.SCAN_CASES if r == "chunked")    # partial chunk,
    assert set(i % 6 for i in range(len(R.SCAN_CASES))) == set(range(6))                    # several ragged tiles


def test_poisoned_envs_sit_mid_tile_and_at_a_tile_edge():
    for i in R.SCAN_SUB:
        route, n, T = R.SCAN_CASES[i]
        w, envs = R.TILE_ENVS[route], R.poisoned_envs(route, n)
        assert len(envs) == 2 and envs[1] < n
        if n >= w:
            assert envs[0] % w == w // 2 and envs[1] % w == w - 1
            assert envs[1] + 1 < n or n % w == 0                     # the edge env has a neighbour in the next tile


@pytest.mark.parametrize("i", range(len(R.SCAN_CASES)), ids=["%s-%d-%d" % c for c in R.SCAN_CASES])
def test_done_bytes_2_and_255_change_the_oracle(i):
    """Reading a done byte as `d == 1` instead of `d != 0` changes the oracle's bits on every case that has a set byte:
    the 2 / 255 bytes of the device test can tell the two apart."""
    x = R.scan_case_inputs(i)
    pattern = R.DONE_PATTERNS[i % 6]
    if pattern == "none":
        assert not x["d"].any()
        return
    vals = set(np.unique(x["d"])) - {0}
    assert 2 in vals and vals <= {1, 2, 255}
    for scan in ("gae", "nstep"):
        right = R.scan_oracle(x, scan, "nep50", 0.99, 0.95)
        wrong = R.scan_oracle(x, scan, "nep50", 0.99, 0.95, done=lambda d: d == 1)
        assert not R.same_bits(right[0], wrong[0]), (scan, pattern)


def test_poison_stays_in_its_env_and_reaches_the_outputs():
    x = R.scan_case_inputs(R.SCAN_SUB[3])
    envs = R.poisoned_envs("lds64x256", x["n"])
    y = R.poison(x, envs)
    for scan in ("gae", "nstep"):
        for _, pname in R.PROMOS:
            clean, bad = R.scan_oracle(x, scan, pname, 0.99, 0.95), R.scan_oracle(y, scan, pname, 0.99, 0.95)
            keep = np.ones(x["n"], bool)
            keep[envs] = False
            for a, b in zip(clean, bad):
                assert R.same_bits(a[keep], b[keep]) and not np.isfinite(b[envs]).all()


# ------------------------------------------------------------------------------------------------ standardise

def _std_inputs():
    for n in R.STD_N:
        for masked in (False, True):
            for eps, ratio, x, valids in R.std_cases(n, masked):
                yield n, masked, eps, ratio, x, valids


def _outside(out, x, valids, eps):
    """Largest |out - reference| / bound over the valid elements (None where var == 0)."""
    sel, y, m, var, d = R.std_reference(x, valids, eps)
    if var == 0:
        return None
    return float((np.abs(out[sel].astype(F64) - y) / R.standardize_bound(y, m, var, d, x.size)).max())


def test_standardize_restatement_stays_inside_the_bound():
    """The kernel's float32 steps restated in NumPy stay inside standardize_bound on exactly the device test's inputs;
    the worst fraction is printed (the device's own is in DESIGN.md section 20)."""
    worst, seen = 0.0, 0
    for n, masked, eps, ratio, x, valids in _std_inputs():
        out = R.std_restatement_f32(x, valids, eps)
        frac = _outside(out, x, valids, eps)
        sel = np.ones(n, bool) if valids is None else valids != 0
        assert R.same_bits(out[~sel], x[~sel])
        if frac is None:
            assert sel.sum() == 1 and R.same_bits(out[sel], np.zeros(1, F32))
            continue
        assert frac <= 1.0, (n, masked, eps, ratio, frac)
        worst, seen = max(worst, frac), seen + 1
    assert seen >= 90
    print("standardise restatement: worst deviation %.3f of the bound over %d inputs" % (worst, seen))


@pytest.mark.parametrize("variant", ["ddof1", "all", "eps_under_root"])
def test_standardize_wrong_variants_leave_the_bound(variant):
    out_of_bound = []
    for n, masked, eps, ratio, x, valids in _std_inputs():
        frac = _outside(R.std_restatement_f32(x, valids, eps, variant), x, valids, eps)
        if frac is not None and frac > 1.0:
            out_of_bound.append((n, masked, eps, ratio))
    assert out_of_bound, variant
    if variant == "ddof1":                                   # even at the largest size (1 / 2n = 4e-6 relative)
        assert any(n >= 131072 for n, _, _, _ in out_of_bound)
    if variant == "all":
        assert all(masked for _, masked, _, _ in out_of_bound)


def test_standardize_denominator_can_be_recovered_from_outputs():
    for n, masked, eps, ratio in ((257, True, 1e-6, 0.0), (131073, False, 0.5, 1e4), (256, False, 1e-6, 1e6)):
        x, valids = R.std_inputs(n, masked, ratio, 5)
        out = R.std_restatement_f32(x, valids, eps)
        sel, y, m, var, d = R.std_reference(x, valids, eps)
        got = R.std_recover_denominator(x[sel], out[sel], m)
        assert got is not None and abs(float(got) - d) <= 4 * R.U32 * d + 1e-3 * d * (ratio >= 1e6)


# --------------------------------------------------------------------------------------------------- sampling

@pytest.mark.parametrize("A", [2, 255, 256])
def test_sampling_ties_tell_less_from_less_or_equal(A):
    p, u = R.sample_inputs(A, 257)
    csum = np.cumsum(p, axis=1, dtype=F32)
    assert (csum[:, -1] == 1).all() and ((p * 1024) % 1 == 0).all()
    kind = np.arange(257) % R.N_U_KINDS
    tie = (kind < 9) & (kind % 3 == 0)
    assert (csum.astype(F64) == u[:, None]).any(axis=1)[tie].all()           # u IS a cumulative sum on those rows
    right, wrong = P.sample_actions(p, u), R.sample_le(p, u)
    assert (right != wrong)[tie & (right < A - 1)].all() and (right != wrong).sum() >= 20
    assert (right == wrong)[(kind % 3 != 0) & (kind < 9)].all()              # one ulp off the tie: both agree
    assert (right[kind == 9] == 0).all() and (right[kind == 10] == (csum < 1).sum(axis=1)[kind == 10]).all()    # u = 0, u = 1
    # rows that sum below u are clamped; a NaN ends the count where it stands
    pe, ue = R.sample_edge_rows(A)
    ke = P.sample_actions(pe, ue)
    assert (ke[:3] == A - 1).all() and ke[3] == 0 and ke[4] == A - 1 and ke[5] == 0


# ------------------------------------------------------------------------------------------ bias + ReLU backward

@pytest.mark.parametrize("channels", R.RELU_CHANNELS)
def test_dbias_restatement_is_not_a_plain_column_sum(channels):
    differ = 0
    for rows in R.RELU_ROWS:
        x, b, dy = R.relu_inputs(rows, channels, 100 + rows)
        s = x + b[None, :]
        y = R.relu_fwd_ref(x, b)
        # what the inputs are there for
        assert ((s == 0) & ~np.signbit(s)).any() and (np.signbit(s) & (s == 0)).any()        # +0 and -0 sums
        assert not np.signbit(y[s == 0]).any()                                               # relu(-0) = +0
        assert ((y == 0) & np.isnan(dy)).any() and not np.isnan(dy[y > 0]).any()
        g = R.relu_bwd_ref(dy, y)
        assert not np.isnan(g).any() and (g[y == 0] == 0).all()
        want = R.dbias_restatement(g)
        exact = g.astype(F64).sum(axis=0)
        scale = np.abs(g).astype(F64).sum(axis=0) + 1e-30
        assert (np.abs(want - exact) <= 64 * R.U32 * scale).all()                # the same sum, to rounding
        differ += not R.same_bits(want, g.sum(axis=0, dtype=F32))
        grid, rpi = R.relu_grid(rows, channels)
        assert grid <= 256 and (grid == 256) == (rows >= 256 * rpi)
    assert differ >= 2, "the restated order must differ from NumPy's own on some of these inputs"
    # the cap binds where the issue says it does
    assert R.relu_grid(21761, 12) == (256, 85) and R.relu_grid(300, 1024) == (256, 1) and R.relu_grid(86, 12) == (2, 85)


def test_gather_tables():
    for rb in R.GATHER_ROW_BYTES:
        obs = R.gather_obs(3, rb, 1)
        assert set(np.unique(obs)) == set(range(256)) or obs.size < 256
    assert set(np.unique(R.gather_obs(17, 16, 1))) == set(range(256))
    idx = R.gather_idx("repeats", 257, 300, 2)
    assert len(set(idx.tolist())) < 257 and idx.max() < 300
    # live lanes of the NHWC gather: one quad, a partly filled wave, a partly filled block
    assert sorted(set(b * p // 4 for p in R.NHWC_PLANE_BYTES for b in R.NHWC_BATCH))[:4] == [4, 12, 20, 60]
