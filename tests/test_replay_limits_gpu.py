"""The replay store and sum-tree kernels (csrc/replay.hip) at the edges of what their entry points accept, through the
_lib wrappers, and the first value past each limit refused.

A. Descent (arl_sumtree_find / arl_sumtree_sample / arl_sumtree_sample_batch) on trees of integer leaves whose root is a
   power of two: u = j / root gives v = j exactly, so v == left occurs at every level (the tie rule is `v > left`,
   sum_tree.py:88-98), and the expected leaf is a closed form -- np.searchsorted on the leaves' running sum -- that
   shares no loop with the kernels.  Depths 1, 2, 3, 11 .. 16: everything in LDS (<= 11), LDS + tail (12), LDS +
   two-level loop (13, 15), LDS + two-level loop + tail (14, 16).  Candidate counts across every thread-count step.
B. arl_is_weights / arl_priority_diffs, the stated arithmetic of the fused copies in the sample and update kernels:
   bit-exact on inputs whose powers are exact (4 ** -k probabilities, squared-integer priorities), one f32 ulp of the
   float64 numpy value otherwise; the fused weights against arl_is_weights bit for bit.
C. arl_sumtree_add against np.add.at (oracle.replay_port.SumTreePort.add) bit for bit on differences whose magnitudes
   span 1e-3 .. 1e16 -- every case is first shown on the CPU to depend on the order of summation -- at every n % 4,
   around the 4096-item chunk seam, and with a node's run of updates starting at every i % 4; arl_sumtree_update_pow
   against both the port and arl_priority_diffs + arl_sumtree_add; arl_sumtree_gather with a scale.
D. arl_replay_append / arl_replay_extract against oracle.replay_port.ReplayPort bit for bit, in both numpy promotions,
   at size == horizon (the mirror of the ring's tail and the newest-frame writes overlap there), horizon 1 and 256,
   reward_horizon 1, 16 and == size, n_stack 2 and 8, frames of 16 bytes and of 257 16-byte chunks; every state of the
   store extracted; and the refusals of every entry point, with nothing written.

Every tolerance that is not equality is the one-f32-ulp bound derived at its test."""
import functools

import numpy as np
import pytest
import torch

from oracle import replay_port as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # (a copy: cached cases are read-only arrays)


def _host(t):
    return t.cpu().numpy()


def _tree_of(leaves):
    """f64[2^levels - 1] with the given leaves and every inner node the sum of its two children."""
    n_leaves = len(leaves)
    tree = np.zeros(2 * n_leaves - 1)
    tree[n_leaves - 1:] = leaves
    for i in range(n_leaves - 2, -1, -1):
        tree[i] = tree[2 * i + 1] + tree[2 * i + 2]
    return tree


# ---------------------------------------------------------------------------------------------------- A. exact ties

TIE_LEVELS = [1, 2, 3, 11, 12, 13, 14, 15, 16]


@functools.lru_cache(maxsize=None)
def _tie_case(levels):
    """-> (tree, root, j, expected tree index per j): integer leaves (about half of them zero), the remainder to a
    power of two on one middle leaf, so every node and every v = j / root * root = j is an exact f64."""
    rs = np.random.RandomState(100 + levels)
    n_leaves = 2 ** (levels - 1)
    leaves = (rs.randint(0, 4, n_leaves) * (rs.rand(n_leaves) < 0.7)).astype(np.float64)
    root = 1
    while root < leaves.sum():
        root *= 2
    leaves[n_leaves // 2] += root - leaves.sum()
    tree = _tree_of(leaves)
    assert tree[0] == root and (tree == np.round(tree)).all()
    if root + 1 <= 4096:
        j = np.arange(root + 1)
    else:
        j = np.concatenate([[0, 1, root - 1, root], rs.choice(np.arange(2, root - 1), 4092, replace=False)])
    j = j[rs.permutation(len(j))]
    assert len(np.unique(j)) == len(j) <= 4096
    leaf = np.where(j >= 1, np.searchsorted(np.cumsum(leaves), j, side="left"), 0)
    assert (leaves[leaf[j >= 1]] > 0).all()                    # a zero-priority leaf is never found
    tree.setflags(write=False), j.setflags(write=False)
    return tree, root, j, leaf + n_leaves - 1


def _run_sample(L, t_dev, tree, levels, u, n, part, batch_kwargs=None):
    """One launch of the sample kernel on canaried outputs; -> (idx, env, step, probs, count) on the host."""
    i32 = lambda: torch.full((n + 2,), -7, dtype=torch.int32, device=DEV)      # noqa: E731
    idx, env, step = i32(), i32(), i32()
    probs = torch.full((n + 2,), -1., dtype=torch.float64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    if batch_kwargs is None:
        L.sumtree_sample(t_dev, levels, u, n, part, idx[:n], env[:n], step[:n], probs[:n], count)
    else:
        L.sumtree_sample_batch(t_dev, levels, u, n, part, idx[:n], env[:n], step[:n], probs[:n], count, **batch_kwargs)
    torch.cuda.synchronize()
    for t in (idx, env, step):
        assert (_host(t)[n:] == -7).all()
    assert (_host(probs)[n:] == -1.).all()
    return _host(idx)[:n], _host(env)[:n], _host(step)[:n], _host(probs)[:n], int(count.item())


def _check_sample(got, tree, levels, want_idx, n, part, what):
    idx, env, step, probs, count = got
    shift = 2 ** (levels - 1) - 1
    uniq = np.unique(want_idx)
    assert count == len(uniq), what
    k = min(count, n)
    full = np.concatenate([uniq[:k], np.full(n - k, uniq[0])])       # the slots past the count repeat the first leaf
    np.testing.assert_array_equal(idx, full, err_msg=what)
    np.testing.assert_array_equal(probs, tree[full], err_msg=what)
    e, s = np.divmod(full - shift, part)
    np.testing.assert_array_equal(env, e, err_msg=what)
    np.testing.assert_array_equal(step, s, err_msg=what)


@pytest.mark.parametrize("levels", TIE_LEVELS)
def test_descent_at_exact_ties(L, levels):
    tree, root, j, want = _tie_case(levels)
    t_dev, u = _dev(tree), _dev(j / root)
    found = torch.full((len(j) + 1,), -7, dtype=torch.int32, device=DEV)
    L.sumtree_find(t_dev, levels, u, found[:len(j)])
    np.testing.assert_array_equal(_host(found)[:len(j)], want)
    assert int(found[len(j)]) == -7
    for part in (1, 7, 2 ** (levels - 1)):
        got = _run_sample(L, t_dev, tree, levels, u, len(j), part)
        _check_sample(got, tree, levels, want, len(j), part, "levels %d part %d" % (levels, part))


@pytest.mark.parametrize("levels", [14, 11])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1024, 1025, 4096])
def test_descent_candidate_counts(L, levels, m):
    """m across every step of the kernel's thread count (64 .. 1024) and up to four candidates per thread."""
    tree, root, j, want = _tie_case(levels)
    sel = np.arange(m) % len(j)                                  # (depth 11 has 2 049 distinct j: they repeat past that)
    t_dev, u = _dev(tree), _dev(j[sel] / root)
    for n in sorted({m, 1}):
        got = _run_sample(L, t_dev, tree, levels, u, n, 7)
        _check_sample(got, tree, levels, want[sel], n, 7, "levels %d m %d n %d" % (levels, m, n))


@pytest.mark.parametrize("ticket", [1, 2 ** 31 - 1])
def test_descent_from_pinned_uniforms_with_notify(L, ticket):
    levels, m = 14, 537
    tree, root, j, want = _tie_case(levels)
    u = torch.from_numpy(j[:m] / root).pin_memory()
    notify = torch.zeros(1, dtype=torch.int64).pin_memory()
    got = _run_sample(L, _dev(tree), tree, levels, u, m, 7, dict(notify=notify, ticket=ticket))
    _check_sample(got, tree, levels, want[:m], m, 7, "pinned")
    assert int(notify[0]) == (ticket << 32) | len(np.unique(want[:m]))


# ---------------------------------------------------------------------------------------------------- B. weights, diffs

def _ulps32(got, want32):
    """|got - want| in f32 ulps of the expected value (np.spacing)."""
    return np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def _is_weights(L, probs, beta):
    out = torch.full((len(probs) + 1,), -1., dtype=torch.float32, device=DEV)
    L.is_weights(_dev(probs), beta, out[:len(probs)])
    assert float(out[len(probs)]) == -1.
    return _host(out)[:len(probs)]


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("beta", [0., 0.5, 1.])
def test_is_weights_exact_family(L, n, beta):
    """probs = 4 ** -k: (1 / p) ** beta / max is a power of two, and the rounding to f32 absorbs a float64 ulp of the
    device's pow.  The largest weight sits once in the first and once in the last slot (a reduction that drops the last
    stride loses the latter)."""
    rs = np.random.RandomState(n)
    for at in (0, n - 1):
        k = rs.randint(0, 20, n)
        k[at] = 20
        probs = 4.0 ** -k
        want = R.importance_weights(probs, beta).astype(np.float32)
        assert want[at] == 1. and (n == 1 or beta == 0 or want.min() < 1.)
        np.testing.assert_array_equal(_is_weights(L, probs, beta), want, err_msg="max at %d" % at)


def test_is_weights_general_beta_within_one_ulp(L, capsys):
    """beta = 0.4, probs in [1e-6, 1] against float64 numpy rounded to f32.  Bound: ONE f32 ulp of the expected value --
    the device's float64 pow and divide are off by float64 ulps, 2^-29 of an f32 ulp, so only a value that straddles an
    f32 rounding boundary can move, and then to the neighbouring f32.  Measured on an MI355X: see LABNOTES.md."""
    rs = np.random.RandomState(4)
    probs = 1e-6 + rs.rand(4097) * (1. - 1e-6)
    want = R.importance_weights(probs, 0.4).astype(np.float32)
    got = _is_weights(L, probs, 0.4)
    err = _ulps32(got, want)
    with capsys.disabled():
        print("\n[is_weights beta=0.4] worst %.3f f32 ulp, %.4f%% of %d not bit-identical"
              % (err.max(), 100. * (got != want).mean(), len(want)))
    assert err.max() <= 1.


def _w_tree(levels, seed):
    rs = np.random.RandomState(seed)
    return _tree_of(4.0 ** -rs.randint(0, 11, 2 ** (levels - 1)))


@pytest.mark.parametrize("levels,m", [(6, 64), (11, 1024), (14, 1025)])
@pytest.mark.parametrize("beta", [0.5, 1.])
def test_fused_weights_equal_is_weights(L, levels, m, beta):
    """arl_sumtree_sample_batch's weights == arl_is_weights on its own probs output, bit for bit, with n distinct leaves;
    with n past the distinct count the weights of the repeated slots are 0."""
    tree = _w_tree(levels, levels)
    t_dev, u = _dev(tree), _dev(np.random.RandomState(m).rand(m))
    count = _run_sample(L, t_dev, tree, levels, u, m, 7)[4]
    assert 1 < count < m                                         # (a birthday collision among m draws is certain here)
    for n in (count, count - 1, m):
        w = torch.full((n + 1,), -1., dtype=torch.float32, device=DEV)
        got = _run_sample(L, t_dev, tree, levels, u, n, 7, dict(beta=beta, is_weights=w[:n]))
        assert got[4] == count and float(w[n]) == -1.
        k = min(n, count)
        probs = got[3][:k]
        assert len(np.unique(got[0][:k])) == k and (np.log2(probs) % 2 == 0).all()      # distinct leaves, 4 ** -k each
        want = _is_weights(L, probs, beta)
        np.testing.assert_array_equal(want, R.importance_weights(probs, beta).astype(np.float32))
        np.testing.assert_array_equal(_host(w)[:k], want)
        assert (_host(w)[k:n] == 0.).all()


def _want_diffs(p32, alpha, last):
    return (p32.astype(np.float64) ** np.float64(np.float32(alpha))).astype(np.float32).astype(np.float64) - last


def _priority_diffs(L, p32, last, alpha):
    out = torch.full((len(p32) + 1,), -7., dtype=torch.float64, device=DEV)
    L.priority_diffs(_dev(p32), _dev(last), alpha, out[:len(p32)])
    assert float(out[len(p32)]) == -7.
    return _host(out)[:len(p32)]


def _square_priorities(rs, n):
    p = (rs.randint(0, 1001, n).astype(np.float64) ** 2).astype(np.float32)
    p[0] = 0. if n > 1 else 49.
    p[-1] = 1000. ** 2
    return p


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("alpha", [0., 0.5, 1.])
def test_priority_diffs_exact_family(L, n, alpha):
    """Squares of the integers 0 .. 1000 as f32: their powers 0, 0.5 and 1 are exact (0 ** 0 == 1)."""
    rs = np.random.RandomState(n + 7)
    p, last = _square_priorities(rs, n), rs.rand(n) * 3
    np.testing.assert_array_equal(_priority_diffs(L, p, last, alpha), _want_diffs(p, alpha, last))


def test_priority_diffs_general_alpha_within_one_ulp(L, capsys):
    """alpha = 0.6 (0.6 as f32, as the kernel takes it), last_probs = 0 so that the difference IS the f32 power.  Bound:
    one f32 ulp of the expected power, by the derivation of test_is_weights_general_beta_within_one_ulp.  Measured on
    an MI355X: see LABNOTES.md."""
    rs = np.random.RandomState(6)
    p = (rs.rand(5000) * 10. ** rs.randint(-4, 3, 5000)).astype(np.float32)
    want = _want_diffs(p, 0.6, 0.)
    got = _priority_diffs(L, p, np.zeros(5000), 0.6)
    assert (got == got.astype(np.float32)).all()
    err = _ulps32(got, want.astype(np.float32))
    with capsys.disabled():
        print("\n[priority_diffs alpha=0.6] worst %.3f f32 ulp, %.4f%% of %d not bit-identical"
              % (err.max(), 100. * (got != want).mean(), len(want)))
    assert err.max() <= 1.


def test_zero_length_calls_launch_nothing(L):
    """n = 0 (arl_priority_diffs, arl_sumtree_gather, arl_sumtree_find, arl_sumtree_add, arl_sumtree_update_pow) and
    batch = 0 (arl_replay_extract) return 0 and write nothing."""
    lib = L.load()
    f64 = torch.full((4,), -7., dtype=torch.float64, device=DEV)
    tree = _dev(_tree_of(np.arange(4.)))
    before = tree.clone()
    p32 = torch.ones(4, device=DEV)
    i32 = torch.full((4,), 3, dtype=torch.int32, device=DEV)
    s = L.stream_ptr()
    L._check(lib.arl_priority_diffs(p32.data_ptr(), f64.data_ptr(), 0, 0.6, f64.data_ptr(), s), "arl_priority_diffs")
    L._check(lib.arl_sumtree_gather(tree.data_ptr(), i32.data_ptr(), 0, -1., f64.data_ptr(), s), "arl_sumtree_gather")
    L._check(lib.arl_sumtree_find(tree.data_ptr(), 3, f64.data_ptr(), 0, i32.data_ptr(), s), "arl_sumtree_find")
    L._check(lib.arl_sumtree_add(tree.data_ptr(), 3, i32.data_ptr(), f64.data_ptr(), 0, s), "arl_sumtree_add")
    L._check(lib.arl_sumtree_update_pow(tree.data_ptr(), 3, i32.data_ptr(), p32.data_ptr(), f64.data_ptr(), 0.6, 0, s),
             "arl_sumtree_update_pow")
    st = _Store(2, 4, 16, 3, 48)
    out = st.extract_outputs(0)
    L._check(lib.arl_replay_extract(st.rb_ref(), i32.data_ptr(), i32.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr(),
                                    out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), s), "arl_replay_extract")
    torch.cuda.synchronize()
    assert (f64 == -7.).all() and (i32 == 3).all() and torch.equal(tree, before)
    st.assert_outputs_untouched(out, 0)


# ---------------------------------------------------------------------------------------------------- C. in-order add

ADD_N = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8193]
ADD_PATTERNS = ["one", "two", "distinct", "random", "run0", "run1", "run2", "run3"]
ADD_CASES = [(1, "one")] + [(lv, p) for lv in (2, 13) for p in ADD_PATTERNS]


def _port_add(tree, levels, idxs, diffs):
    """SumTreePort.add (np.add.at per level, sum_tree.py:54-57) on a copy of `tree`."""
    ref = R.SumTreePort.__new__(R.SumTreePort)
    ref.level, ref.tree = levels, tree.copy()
    ref.add(idxs, diffs)
    return ref.tree


def _add_leaves(pattern, n, n_leaves, rs):
    """Leaf of every item, or None where the pattern does not exist at this size."""
    if pattern == "one":
        return np.full(n, n_leaves // 2)
    if pattern == "two":
        return np.where(np.arange(n) % 2 == 0, n_leaves - 1, 0)
    if pattern == "distinct":
        return rs.permutation(n_leaves)[:n] if n <= n_leaves else None
    if pattern == "random":
        return rs.randint(0, min(n_leaves, 37), n)              # heavy repetition
    r = int(pattern[3])                                          # a run on leaf 0 whose first item sits at i % 4 == r
    start = r + (8 if n > 64 else 0)
    if start >= n:
        return None
    leaves = 1 + (rs.permutation(n_leaves - 1)[:n] if n <= n_leaves - 1 else rs.randint(0, n_leaves - 1, n))
    offs = np.array([0, 1, 2, 3, 4, 5, 7, 8, 11, 16, 17, 18, 19, 20, 29, 4087, 4088, 4089, n - 2 - start, n - 1 - start])
    leaves[start + offs[(offs >= 0) & (offs < n - start)]] = 0
    return leaves


def _add_case(levels, pattern, n):
    """-> (tree, idxs, diffs, expected tree) for which the order of summation shows in the bits: the same items added in
    reversed order give a different tree (asserted; the seed is the first for which it holds).  n == 1 has no order."""
    n_leaves = 2 ** (levels - 1)
    for seed in range(64):
        rs = np.random.RandomState(1000 * levels + 64 * n + seed)
        tree = _tree_of(rs.rand(n_leaves) * 100)
        leaves = _add_leaves(pattern, n, n_leaves, rs)
        if leaves is None:
            return None
        idxs = (leaves + n_leaves - 1).astype(np.int32)
        diffs = rs.choice([1e16, -1e16, 1., -1., 1e-3, -1e-3], n) * rs.randn(n)
        want = _port_add(tree, levels, idxs, diffs)
        if n == 1 or not np.array_equal(want, _port_add(tree, levels, idxs[::-1], diffs[::-1])):
            return tree, idxs, diffs, want
    raise AssertionError("no seed makes levels %d %s n %d depend on the order" % (levels, pattern, n))


@pytest.mark.parametrize("levels,pattern", ADD_CASES, ids=lambda v: str(v))
def test_sumtree_add_in_input_order(L, levels, pattern):
    ran = 0
    for n in ADD_N:
        case = _add_case(levels, pattern, n)
        if case is None:
            continue
        tree, idxs, diffs, want = case
        t = _dev(tree)
        L.sumtree_add(t, levels, _dev(idxs), _dev(diffs))
        np.testing.assert_array_equal(_host(t), want, err_msg="n %d" % n)
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize("n", [6, 4096, 4097])
@pytest.mark.parametrize("alpha", [0., 0.5, 1.])
def test_sumtree_update_pow_with_duplicates(L, n, alpha):
    """The fused update == SumTreePort.add of the stated differences == arl_priority_diffs + arl_sumtree_add, bit for
    bit, on leaves that repeat, across the chunk seam."""
    levels, n_leaves = 13, 4096
    rs = np.random.RandomState(n + int(10 * alpha))
    tree = _tree_of(rs.rand(n_leaves) * 1e6)
    idxs = (rs.randint(0, max(3, n // 8), n) * 5 + n_leaves - 1).astype(np.int32)
    assert len(np.unique(idxs)) < n
    p, last = _square_priorities(rs, n), rs.rand(n) * 10. ** rs.randint(-3, 14, n)    # (magnitudes apart: order shows)
    diffs = _want_diffs(p, alpha, last)
    want = _port_add(tree, levels, idxs, diffs)
    assert not np.array_equal(want, _port_add(tree, levels, idxs[::-1], diffs[::-1]))
    fused, split = _dev(tree), _dev(tree)
    L.sumtree_update_pow(fused, levels, _dev(idxs), _dev(p), _dev(last), alpha)
    d = torch.empty(n, dtype=torch.float64, device=DEV)
    L.priority_diffs(_dev(p), _dev(last), alpha, d)
    L.sumtree_add(split, levels, _dev(idxs), d)
    np.testing.assert_array_equal(_host(d), diffs)
    np.testing.assert_array_equal(_host(fused), want)
    np.testing.assert_array_equal(_host(split), want)


@pytest.mark.parametrize("n", [1, 256, 257])
def test_sumtree_gather_scaled(L, n):
    levels, n_leaves = 13, 4096
    rs = np.random.RandomState(n)
    tree = _tree_of(rs.rand(n_leaves))
    idxs = rs.randint(0, 2 * n_leaves - 1, n).astype(np.int32)
    idxs[0], idxs[-1] = 2 * n_leaves - 2, 0
    out = torch.full((n + 1,), -7., dtype=torch.float64, device=DEV)
    L.sumtree_gather(_dev(tree), _dev(idxs), out[:n], scale=-1.)
    np.testing.assert_array_equal(_host(out)[:n], -tree[idxs])
    assert float(out[n]) == -7.


# ---------------------------------------------------------------------------------------------------- D. the frame store

STORE_SHAPES = [
    # (n_env, n_stack, horizon, env_size, reward_horizon, frame_bytes)
    (2, 4, 16, 16, 3, 4112),       # size == horizon, 257 chunks: mirror and newest-frame writes overlap across waves
    (8, 4, 4, 4, 3, 4112),         # size == horizon, more workgroups
    (3, 2, 256, 256, 16, 16),      # largest horizon, smallest stack and frame
    (2, 4, 1, 16, 16, 48),         # horizon 1, reward_horizon == size
    (2, 4, 2, 8, 1, 48),           # reward_horizon 1: returns == rewards
    (2, 3, 16, 32, 16, 32),        # largest reward horizon with wrap
    (2, 8, 4, 16, 3, 16),          # deep stack: blank ramps up to 7
]
N_APPENDS, DISCOUNT, SPARE = 5, 0.99, 3
STORE_KEYS = ("frames", "n_blanks", "acts", "terminals", "rewards", "returns")


class _Store(object):
    """The device arrays of one arl_replay and its struct, as FrameReplayBuffer lays them out."""

    def __init__(self, n_env, n_stack, size, reward_horizon, frame_bytes, fill=0):
        from accel_rl_amd import _lib
        self.E, self.F, self.S, self.P = n_env, n_stack, size, frame_bytes
        ring = size + n_stack - 1
        mk = lambda shape, dt: torch.full(shape, fill, dtype=dt, device=DEV)      # noqa: E731
        self.frames, self.n_blanks = mk((n_env, ring, frame_bytes), torch.uint8), mk((n_env, ring), torch.uint8)
        self.acts, self.terminals = mk((n_env, size), torch.uint8), mk((n_env, size), torch.uint8)
        self.rewards, self.returns = mk((n_env, size), torch.float32), mk((n_env, size), torch.float32)
        self.rb = rb = _lib.ArlReplay()
        rb.n_env, rb.size, rb.n_stack, rb.frame_bytes, rb.reward_horizon = n_env, size, n_stack, frame_bytes, reward_horizon
        for k in STORE_KEYS:
            setattr(rb, k, getattr(self, k).data_ptr())

    def rb_ref(self):
        import ctypes
        return ctypes.byref(self.rb)

    def arrays(self):
        return {k: _host(getattr(self, k)).copy() for k in STORE_KEYS}

    def extract_outputs(self, batch):
        """Canaried outputs with SPARE rows past the batch."""
        rows = batch + SPARE
        return (torch.full((rows, self.F, self.P), 0xAB, dtype=torch.uint8, device=DEV),
                torch.full((rows, self.F, self.P), 0xAB, dtype=torch.uint8, device=DEV),
                torch.full((rows,), 0xAB, dtype=torch.uint8, device=DEV),
                torch.full((rows,), -777., dtype=torch.float32, device=DEV),
                torch.full((rows,), 0xAB, dtype=torch.uint8, device=DEV))

    @staticmethod
    def assert_outputs_untouched(out, batch):
        for t, v in zip(out, (0xAB, 0xAB, 0xAB, -777., 0xAB)):
            assert bool((t[batch:] == v).all())

    def extract(self, L, env_idxs, step_idxs):
        b = len(env_idxs)
        out = self.extract_outputs(b)
        L.replay_extract(self.rb, _dev(np.asarray(env_idxs, np.int32)), _dev(np.asarray(step_idxs, np.int32)),
                         *[t[:b] for t in out])
        torch.cuda.synchronize()
        self.assert_outputs_untouched(out, b)
        return [_host(t)[:b] for t in out]


def _port_arrays(port):
    d = {k: getattr(port, k).copy() for k in STORE_KEYS}
    d["terminals"] = d["terminals"].astype(np.uint8)
    return d


@functools.lru_cache(maxsize=None)
def _store_reference(shape):
    """The appended batches and, per promotion, ReplayPort's arrays after every append and its extraction of every
    state -- computed once, shared by both parametrisations."""
    E, F, T, S, h_r, P = shape
    rs = np.random.RandomState(sum(shape))
    batches = []
    for _ in range(N_APPENDS):
        dones = rs.rand(E, T) < 0.05
        dones[0], dones[1] = True, False                         # one environment all done, one never
        batches.append((rs.randint(0, 256, (E, T, F, P), dtype=np.uint8), rs.randint(0, 18, (E, T)).astype(np.uint8),
                        (rs.randn(E, T) * 10. ** rs.randint(-3, 6, (E, T))).astype(np.float32), dones))
    env_idxs, step_idxs = np.repeat(np.arange(E), S), np.tile(np.arange(S), E)
    ref = dict()
    for promo in ("nep50", "legacy"):
        port = R.ReplayPort(E, F, (P,), E * S, h_r, T, DISCOUNT, promo=promo)
        assert port.S == S
        after = []
        for b in batches:
            port.append(*b)
            after.append(_port_arrays(port))
        ref[promo] = (after, [np.asarray(x) for x in port.extract_batch(env_idxs, step_idxs)], port)
    nep, leg = ref["nep50"][0][-1], ref["legacy"][0][-1]
    if h_r > 1:      # the two promotions must be told apart by this shape's data, or one parametrisation proves nothing
        assert not np.array_equal(nep["returns"], leg["returns"])
    else:            # a one-step return is the reward itself in either promotion
        assert np.array_equal(nep["returns"], nep["rewards"]) and np.array_equal(leg["returns"], leg["rewards"])
    assert nep["terminals"].any() and not nep["terminals"].all()
    return batches, env_idxs, step_idxs, ref


def _append(L, st, batch, T, idx, promo):
    obs, acts, rews, dones = batch
    L.replay_append(st.rb, _dev(obs.reshape((-1,) + obs.shape[2:])), _dev(acts.reshape(-1)), _dev(rews.reshape(-1)),
                    _dev(dones.reshape(-1).astype(np.uint8)), T, idx, DISCOUNT, promo)


@pytest.mark.parametrize("promo", ["nep50", "legacy"])
@pytest.mark.parametrize("shape", STORE_SHAPES, ids=lambda s: "E%d-F%d-T%d-S%d-h%d-P%d" % s)
def test_store_at_its_bounds(L, shape, promo):
    E, F, T, S, h_r, P = shape
    batches, env_idxs, step_idxs, ref = _store_reference(shape)
    after, want_x, _ = ref[promo]
    st = _Store(E, F, S, h_r, P)
    idx = 0
    for b, batch in enumerate(batches):
        _append(L, st, batch, T, idx, L.PROMO_NEP50 if promo == "nep50" else L.PROMO_LEGACY)
        idx = (idx + T) % S
        got = st.arrays()
        for k in STORE_KEYS:
            np.testing.assert_array_equal(got[k], after[b][k], err_msg="append %d: %s" % (b, k))
    got_x = st.extract(L, env_idxs, step_idxs)                   # every state of the store
    for name, g, w in zip(("obs", "next_obs", "actions", "returns", "terminals"), got_x, want_x):
        np.testing.assert_array_equal(g, w.astype(g.dtype), err_msg=name)


@pytest.mark.parametrize("pairs", [[(1, 5)], [(0, 15)] * 64], ids=["batch1", "64copies"])
def test_extract_small_and_repeated_batches(L, pairs):
    shape = STORE_SHAPES[6]
    E, F, T, S, h_r, P = shape
    batches, _, _, ref = _store_reference(shape)
    port = ref["nep50"][2]
    st = _Store(E, F, S, h_r, P)
    for b, batch in enumerate(batches):
        _append(L, st, batch, T, (b * T) % S, L.PROMO_NEP50)
    e, s = np.array(pairs).T
    for g, w in zip(st.extract(L, e, s), port.extract_batch(e, s)):
        np.testing.assert_array_equal(g, np.asarray(w).astype(g.dtype))


# ---------------------------------------------------------------------------------------------------- refusals

E_ARG, E_RANGE, E_ALIGN = -1, -2, -3           # include/accel_rl_hip.h


def _refused(call, code, match):
    with pytest.raises(RuntimeError, match=r"\(code %d\): .*%s" % (code, match)):
        call()


def test_store_refuses_past_its_limits(L):
    """Every refusal comes from the entry point's own checks (before any launch) and leaves the store and the outputs
    as they were.  The arrays are those of a (2, 4, 16, 3, 48) store; the struct's fields are then set past each limit."""
    E, F, S, h_r, P, T = 2, 4, 16, 3, 48, 4
    st = _Store(E, F, S, h_r, P, fill=0x5A)
    before = st.arrays()
    obs = torch.zeros(E * 256 * F * P + 16, dtype=torch.uint8, device=DEV)      # (large enough for any horizon <= 256)
    acts = torch.zeros(E * 256, dtype=torch.uint8, device=DEV)
    rews = torch.zeros(E * 256, device=DEV)
    good = dict(size=S, n_stack=F, frame_bytes=P, reward_horizon=h_r)

    def append(horizon=T, idx=0, promo=L.PROMO_NEP50, o=obs[:-16], **fields):
        for k, v in dict(good, **fields).items():
            setattr(st.rb, k, v)
        try:
            L.replay_append(st.rb, o, acts, rews, acts, horizon, idx, DISCOUNT, promo)
        finally:
            for k, v in good.items():
                setattr(st.rb, k, v)

    out = st.extract_outputs(4)
    idxs = torch.zeros(4, dtype=torch.int32, device=DEV)

    def extract(o=None, no=None, **fields):
        for k, v in dict(good, **fields).items():
            setattr(st.rb, k, v)
        try:
            L.replay_extract(st.rb, idxs, idxs, out[0][:4] if o is None else o, out[1][:4] if no is None else no,
                             out[2][:4], out[3][:4], out[4][:4])
        finally:
            for k, v in good.items():
                setattr(st.rb, k, v)

    store_limits = "need n_stack >= 2, frame_bytes % 16 == 0, 1 <= reward_horizon <= 16"
    for fields, what in ((dict(frame_bytes=24), store_limits), (dict(n_stack=1), store_limits),
                         (dict(reward_horizon=0), store_limits), (dict(reward_horizon=17, size=32), store_limits),
                         (dict(reward_horizon=9, size=8), store_limits),             # reward_horizon > size
                         (dict(size=2, reward_horizon=2), "size >= n_stack - 1")):  # the mirror would overlap itself
        _refused(lambda: append(horizon=1, **fields), E_RANGE, what)
        _refused(lambda: extract(**fields), E_RANGE, what)
    ring_limits = "size must be a multiple of horizon \\(<= 256\\), idx a multiple of it"
    for kw in (dict(horizon=0), dict(horizon=257), dict(horizon=5),                 # 16 % 5 != 0
               dict(horizon=4, idx=3), dict(horizon=4, idx=16), dict(horizon=8, idx=12), dict(horizon=4, idx=-4)):
        _refused(lambda: append(**kw), E_RANGE, ring_limits)
    _refused(lambda: append(promo=7), E_ARG, "bad promo")
    _refused(lambda: append(o=obs[1:-15]), E_ALIGN, "observations must be 16-byte aligned")
    flat = torch.full((4 * F * P + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    _refused(lambda: extract(o=flat[1:1 + 4 * F * P]), E_ALIGN, "obs buffers must be 16-byte aligned")
    _refused(lambda: extract(no=flat[1:1 + 4 * F * P]), E_ALIGN, "obs buffers must be 16-byte aligned")
    torch.cuda.synchronize()
    after = st.arrays()
    for k in STORE_KEYS:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    st.assert_outputs_untouched(out, 0)
    assert bool((flat == 0xAB).all())
    # the struct is back at its accepted values: the same calls now run
    append()
    extract()
    torch.cuda.synchronize()
    assert not np.array_equal(st.arrays()["acts"], before["acts"])


def test_sumtree_refuses_past_its_limits(L):
    lib = L.load()
    levels = 4
    tree = _dev(_tree_of(np.arange(1., 9.)))
    before = tree.clone()
    u = torch.rand(4097, dtype=torch.float64, device=DEV)
    i32 = lambda n=8: torch.full((n,), -7, dtype=torch.int32, device=DEV)      # noqa: E731
    idx, env, step, count, found = i32(), i32(), i32(), i32(1), i32()
    probs = torch.full((8,), -1., dtype=torch.float64, device=DEV)
    w = torch.full((8,), -1., dtype=torch.float32, device=DEV)
    diffs = torch.ones(8, dtype=torch.float64, device=DEV)
    pri = torch.ones(8, device=DEV)
    leaves = torch.full((8,), 7, dtype=torch.int32, device=DEV)
    notify = torch.zeros(2, dtype=torch.int64).pin_memory()
    s = L.stream_ptr()

    def sample(levels=levels, m=8, n=4, part=3):
        L.sumtree_sample(tree, levels, u[:m], n, part, idx, env, step, probs, count)

    def sample_batch(levels=levels, m=8, n=4, part=3, notify_at=0):
        L._check(lib.arl_sumtree_sample_batch(tree.data_ptr(), levels, u.data_ptr(), m, n, part, idx.data_ptr(),
                                              env.data_ptr(), step.data_ptr(), probs.data_ptr(), count.data_ptr(), 0.5,
                                              w.data_ptr(), notify.data_ptr() + notify_at, 1, s), "arl_sumtree_sample_batch")

    candidates = "need 1 <= n <= m <= 4096 candidates"
    for kw in (dict(levels=0), dict(levels=32), dict(m=4097), dict(m=4, n=5), dict(n=0), dict(part=0)):
        _refused(lambda: sample(**kw), E_RANGE, candidates)
        _refused(lambda: sample_batch(**kw), E_RANGE, candidates)
    for at in (1, 4):
        _refused(lambda: sample_batch(notify_at=at), E_ALIGN, "notify: 8-byte aligned")
    for lv in (0, 32):
        _refused(lambda: L.sumtree_find(tree, lv, u[:8], found), E_RANGE, "bad levels / n")
        _refused(lambda: L.sumtree_add(tree, lv, leaves, diffs), E_RANGE, "bad levels / n")
        _refused(lambda: L.sumtree_update_pow(tree, lv, leaves, pri, diffs, 0.6), E_RANGE, "bad levels / n")
    _refused(lambda: L._check(lib.arl_is_weights(probs.data_ptr(), 0, 0.5, w.data_ptr(), s), "arl_is_weights"),
             E_RANGE, "bad n")
    torch.cuda.synchronize()
    assert torch.equal(tree, before) and int(notify[0]) == 0 and int(notify[1]) == 0
    for t in (idx, env, step, count, found):
        assert bool((t == -7).all())
    assert bool((probs == -1.).all()) and bool((w == -1.).all())
    sample()                                                     # the accepted values run
    sample_batch()
    torch.cuda.synchronize()
    assert int(count[0]) >= 1 and int(notify[0]) == (1 << 32) | int(count[0])
