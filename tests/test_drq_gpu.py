"""DrQ on the device: the shifted extraction gather (csrc/replay.hip: arl_replay_extract_shift), the K/M-averaged loss
(csrc/dqn.hip: arl_drq_loss), AtariDqnPolicy.drq_loss_and_grads, DrQ and `augment_args` of the rest of the family.  The
reference has none of it; the yardsticks are tests/drq_ref.py's restatements: the gather is integer-exact, the loss is
compared bit for bit with the fp32 emulation and within the derived bound (drq_ref's docstring) with
float64.  Outputs are prefilled with sentinels; the padding columns of every loss input hold 1e9."""
import functools
import re

import numpy as np
import pytest
import torch

import drq_ref as dr
from test_munchausen_gpu import _make_policy, _ref_params, _ref_q
from test_replay_limits_gpu import E_ALIGN, E_ARG, E_RANGE, _append, _Store

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GAMMA = float(np.float32(0.99 ** 3))


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- extraction ------------------------------------------------------------------------------------------------------

N_ENV, HORIZON, SIZE, H_R = 2, 4, 12, 3
SEED, CALL = -5, 2 ** 33 + 7                    # a negative seed and a call counter that needs its high word


@functools.lru_cache(maxsize=None)
def _filled(n_stack, h, w):
    """A (2 env, 12 state, reward horizon 3) store of h x w frames after five appends of seeded bytes through
    arl_replay_append (the ring has wrapped; env 0 finished an episode two steps before the write cursor, so its newest
    states sit inside the blank-frame window).  -> (_Store, NumPy copies of its arrays)."""
    from accel_rl_amd import _lib
    st = _Store(N_ENV, n_stack, SIZE, H_R, h * w)
    rs = np.random.RandomState(h * w + n_stack)
    idx = 0
    for n in range(5):
        dones = rs.rand(N_ENV, HORIZON) < 0.15
        if n == 4:
            dones[0] = [False, True, False, False]
        batch = (rs.randint(0, 256, (N_ENV, HORIZON, n_stack, h * w), dtype=np.uint8),
                 rs.randint(0, 18, (N_ENV, HORIZON)).astype(np.uint8), rs.randn(N_ENV, HORIZON).astype(np.float32), dones)
        _append(_lib, st, batch, HORIZON, idx, _lib.PROMO_NEP50)
        idx = (idx + HORIZON) % SIZE
    torch.cuda.synchronize()
    arrays = st.arrays()
    for a in arrays.values():
        a.setflags(write=False)
    return st, arrays


def _samples(arrays, batch):
    """(env, step) pairs: first a sample inside the blank window whose next observation wraps the ring, then one per
    remaining blank count, the last state (its next observation wraps), state 0, then seeded pairs."""
    nb = arrays["n_blanks"][:, :SIZE]
    blank = [tuple(p) for p in np.argwhere(nb > 0)]
    assert blank and len({int(nb[p]) for p in blank}) >= 1
    wrap_blank = [p for p in blank if p[1] + H_R >= SIZE]
    head = (wrap_blank[:1] or blank[:1]) + blank + [(1, SIZE - 1), (0, 0)]
    rs = np.random.RandomState(batch)
    pairs = (head + [(rs.randint(N_ENV), rs.randint(SIZE)) for _ in range(batch)])[:batch]
    assert any(s + H_R >= SIZE for _, s in pairs) or batch == 1
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


SPARE = 2


def _outputs(st, h, w, batch, m, k):
    """Sentinel-filled outputs with SPARE rows past each."""
    u8 = lambda *shape: torch.full(shape, 0xAB, dtype=torch.uint8, device=DEV)      # noqa: E731
    return (u8(m * batch + SPARE, st.F, h, w), u8(k * batch + SPARE, st.F, h, w), u8(batch + SPARE),
            torch.full((batch + SPARE,), -777., device=DEV), u8(batch + SPARE))


def _untouched(out, rows):
    return all(bool((t[r:] == v).all()) for t, r, v in zip(out, rows, (0xAB, 0xAB, 0xAB, -777., 0xAB)))


def _extract_shift(L, st, h, w, env, step, pad, m, k, seed=SEED, call=CALL):
    b = len(env)
    out = _outputs(st, h, w, b, m, k)
    rows = (m * b, k * b, b, b, b)
    L.replay_extract_shift(st.rb, _dev(env), _dev(step), h, w, pad, m, k, seed, call, *[t[:r] for t, r in zip(out, rows)])
    torch.cuda.synchronize()
    assert _untouched(out, rows)
    return [t[:r].cpu().numpy() for t, r in zip(out, rows)]


def _want(arrays, n_stack, h, w, env, step, pad, m, k, seed=SEED, call=CALL):
    return dr.shifted_extract(arrays, SIZE, n_stack, H_R, h, w, env, step, pad, m, k, seed, call)


NAMES = ("obs", "next_obs", "actions", "returns", "terminals")


@pytest.mark.parametrize("views", [(1, 1), (2, 3), (8, 8)], ids=lambda v: "M%d-K%d" % v)
@pytest.mark.parametrize("batch", [1, 33])
@pytest.mark.parametrize("n_stack", [2, 4])
@pytest.mark.parametrize("shape", [(4, 4), (8, 16), (104, 80)], ids=lambda s: "%dx%d" % s)
def test_shifted_extraction_bit_for_bit(L, shape, n_stack, batch, views):
    """(4, 4) at pad 4: every index clamps.  One workgroup per view: 2 .. 528 of them."""
    h, w = shape
    m, k = views
    st, arrays = _filled(n_stack, h, w)
    env, step = _samples(arrays, batch)
    got = _extract_shift(L, st, h, w, env, step, 4, m, k)
    want = _want(arrays, n_stack, h, w, env, step, 4, m, k)
    for name, g, x in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, x.astype(g.dtype), err_msg=name)
    if batch == 33:
        assert (arrays["n_blanks"][env, step] > 0).any() and not got[0][0, 0].any()     # a blank frame stays all zero
        assert len({tuple(o) for o in want[5].reshape(-1, 2)}) > 8


@pytest.mark.parametrize("shape", [(264, 64), (20, 1024)], ids=lambda s: "%dx%d" % s)
def test_frames_above_one_tile_are_staged_in_row_tiles(L, shape):
    """16 896 and 20 480 bytes per frame: 252 + 12 and 12 + 8 rows per tile."""
    h, w = shape
    st, arrays = _filled(2, h, w)
    env, step = _samples(arrays, 5)
    for pad in (4, 64):
        got = _extract_shift(L, st, h, w, env, step, pad, 2, 1)
        want = _want(arrays, 2, h, w, env, step, pad, 2, 1)
        assert np.abs(want[5]).max() > 2
        for name, g, x in zip(NAMES, got, want):
            np.testing.assert_array_equal(g, x.astype(g.dtype), err_msg="%s pad %d" % (name, pad))


@pytest.mark.parametrize("n_stack,shape", [(2, (4, 4)), (4, (8, 16)), (4, (104, 80))])
def test_pad_0_is_the_plain_extraction_bit_for_bit(L, n_stack, shape):
    h, w = shape
    st, arrays = _filled(n_stack, h, w)
    env, step = _samples(arrays, 33)
    got = _extract_shift(L, st, h, w, env, step, 0, 1, 1)
    plain = st.extract(L, env, step)
    for name, g, x in zip(NAMES, got, plain):
        np.testing.assert_array_equal(g.reshape(x.shape), x, err_msg=name)
    views = _extract_shift(L, st, h, w, env, step, 0, 3, 2)     # every view of an unshifted extraction is the same
    for v in range(3):
        np.testing.assert_array_equal(views[0][v * 33:(v + 1) * 33], got[0])
    for v in range(2):
        np.testing.assert_array_equal(views[1][v * 33:(v + 1) * 33], got[1])


def test_offsets_per_view_and_determinism(L):
    n_stack, h, w, b = 4, 8, 16, 33
    st, arrays = _filled(n_stack, h, w)
    env, step = _samples(arrays, b)
    got = _extract_shift(L, st, h, w, env, step, 4, 8, 8)
    offs = _want(arrays, n_stack, h, w, env, step, 4, 8, 8)[5]
    frames = arrays["frames"].reshape(N_ENV, -1, h, w)
    for v in range(16):                         # every frame of a view moved by the view's ONE offset
        for j in range(b):
            i = (step[j] + H_R) % SIZE if v >= 8 else step[j]
            dx, dy = offs[v, j]
            for f in range(arrays["n_blanks"][env[j], i], n_stack):
                padded = np.pad(frames[env[j], i + f], 4, mode="edge")
                view = (got[1] if v >= 8 else got[0])[(v % 8) * b + j, f]
                assert np.array_equal(view, padded[4 + dy:4 + dy + h, 4 + dx:4 + dx + w])
    for j in range(b):                          # the views of one sample do not share their offset
        assert len({tuple(o) for o in offs[:, j]}) >= 2
    assert not np.array_equal(got[0][:b], got[0][b:2 * b])
    again = _extract_shift(L, st, h, w, env, step, 4, 8, 8)
    later = _extract_shift(L, st, h, w, env, step, 4, 8, 8, call=CALL + 1)
    other = _extract_shift(L, st, h, w, env, step, 4, 8, 8, seed=SEED + 1)
    for x, y in zip(got, again):
        assert np.array_equal(x, y)
    for changed in (later, other):
        assert not np.array_equal(got[0], changed[0]) and not np.array_equal(got[1], changed[1])
        for x, y in zip(got[2:], changed[2:]):
            assert np.array_equal(x, y)


def test_extraction_refusals_write_nothing(L):
    lib = L.load()
    n_stack, h, w, b = 4, 8, 16, 4
    st, _ = _filled(n_stack, h, w)
    out = _outputs(st, h, w, b, 8, 8)
    idx = torch.zeros(b, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def call(env=p(idx), step=p(idx), batch=b, fh=h, fw=w, pad=4, m=1, k=1, obs=p(out[0]), nxt=p(out[1]), acts=p(out[2]),
             rets=p(out[3]), terms=p(out[4]), **fields):
        keep = {f: getattr(st.rb, f) for f in fields}
        for f, v in fields.items():
            setattr(st.rb, f, v)
        try:
            return lib.arl_replay_extract_shift(st.rb_ref(), env, step, batch, fh, fw, pad, m, k, SEED, CALL, obs, nxt, acts,
                                                rets, terms, None)
        finally:
            for f, v in keep.items():
                setattr(st.rb, f, v)

    for kw in (dict(env=None), dict(step=None), dict(obs=None), dict(nxt=None), dict(acts=None), dict(rets=None),
               dict(terms=None)):
        assert call(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw, what in ((dict(batch=0), b"batch"), (dict(batch=2 ** 31), b"batch"), (dict(fh=8, fw=12), b"frame_bytes"),
                     (dict(fh=16, fw=16), b"frame_bytes"), (dict(fh=0, fw=0), b"frame_bytes"),
                     (dict(fh=64, fw=2), b"multiple of 4"), (dict(fh=2, fw=64, pad=70), b"pad"),
                     (dict(pad=-1), b"pad"), (dict(pad=65), b"pad"), (dict(m=0), b"m_obs"), (dict(m=9), b"m_obs"),
                     (dict(k=0), b"k_next"), (dict(k=9), b"k_next"), (dict(batch=2 ** 27, m=8, k=8), b"2\\^31"),
                     (dict(fh=4, fw=8192, frame_bytes=32768), b"4088")):
        assert call(**kw) == E_RANGE, kw
        assert re.search(what, lib.arl_last_error()), (kw, lib.arl_last_error())
    assert call(obs=p(out[0]) + 4) == E_ALIGN and call(nxt=p(out[1]) + 8) == E_ALIGN
    torch.cuda.synchronize()
    assert _untouched(out, (0, 0, 0, 0, 0))
    assert call(pad=64, m=8, k=8) == 0 and call(batch=1, pad=0) == 0    # at the limits it runs
    torch.cuda.synchronize()
    assert not _untouched(out, (0, 0, 0, 0, 0)) and _untouched(out, (8 * b, 8 * b, b, b, b))


# ---- loss ------------------------------------------------------------------------------------------------------------

def _launch(L, c, gamma_n, delta_clip, baseline=False):
    """baseline: arl_dqn_loss on the same (k = m = 1) rows."""
    q = _dev(c["q"])
    bsz = c["batch"]
    dq = torch.full_like(q, NAN)
    rows, td = torch.full((bsz,), NAN, device=DEV), torch.full((bsz,), NAN, device=DEV)
    args = (q, _dev(c["nxt"]), _dev(c["pol"]), _dev(c["act"]), _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), c["n_act"],
            gamma_n, delta_clip)
    if baseline:
        L.dqn_loss(*args, dq, rows, td, dueling=c["dueling"])
    else:
        L.drq_loss(*args, c["m"], c["k"], dq, rows, td, dueling=c["dueling"])
    torch.cuda.synchronize()
    return dq.cpu().numpy(), rows.cpu().numpy(), td.cpu().numpy()


SHAPES = [(4, 1), (18, 37), (64, 5)]
FLAGS = [(duel, dbl, wtd, clip) for duel in (False, True) for dbl in (False, True) for wtd in (False, True)
         for clip in (1.0, 0.25, 0.0)]


def _seed(a, b, duel, dbl, wtd, clip, k, m):
    return 1000 * a + 10 * b + 4 * duel + 2 * dbl + wtd + int(100 * clip) + 7 * k + 13 * m


def _dq_is_zero_outside_the_taken_entries(c, dq):
    a, bsz, cols = c["n_act"], c["batch"], c["n_act"] + int(c["dueling"])
    assert not dq[:, cols:].any()                               # the padding columns
    if not c["dueling"]:
        other = np.ones((c["m"] * bsz, a), bool)
        other[np.arange(c["m"] * bsz), np.tile(c["act"], c["m"])] = False
        assert not dq[:, :a][other].any()


@pytest.mark.parametrize("n_act,batch", SHAPES)
def test_k_m_1_equals_the_dqn_loss_bit_for_bit(L, n_act, batch):
    for duel, dbl, wtd, clip in FLAGS:
        c = dr.drq_case(_seed(n_act, batch, duel, dbl, wtd, clip, 1, 1), n_act, batch, 1, 1, duel, dbl, wtd, delta_clip=clip,
                        special=True)
        got, want = _launch(L, c, GAMMA, clip), _launch(L, c, GAMMA, clip, baseline=True)
        assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 0
        for x, y in zip(got, want):
            assert np.array_equal(x, y), (duel, dbl, wtd, clip)
        for x, y in zip(got, dr.emu_dqn32(c, GAMMA, clip)):     # (and both are what the emulation says)
            assert np.array_equal(x, y), (duel, dbl, wtd, clip)


@pytest.mark.parametrize("k,m", [(2, 2), (1, 3), (8, 8)])
@pytest.mark.parametrize("n_act,batch", SHAPES)
def test_loss_equals_the_fp32_emulation_bit_for_bit(L, n_act, batch, k, m):
    """Rows with two equal maxima and rows at |d| == delta_clip exactly included (drq_case(special=True))."""
    for duel, dbl, wtd, clip in FLAGS:
        c = dr.drq_case(_seed(n_act, batch, duel, dbl, wtd, clip, k, m), n_act, batch, k, m, duel, dbl, wtd, delta_clip=clip,
                        special=True)
        got = _launch(L, c, GAMMA, clip)
        for name, x, y in zip(("dq", "loss_rows", "td_abs"), got, dr.emu_drq32(c, GAMMA, clip)):
            assert np.array_equal(x, y), (name, duel, dbl, wtd, clip)
        if clip > 0:
            assert (got[2][0::5] == np.float32(clip)).all()
        _dq_is_zero_outside_the_taken_entries(c, got[0])


@pytest.mark.parametrize("k,m", [(1, 1), (2, 2), (1, 3), (8, 8)])
@pytest.mark.parametrize("n_act,batch", SHAPES)
def test_loss_within_the_derived_bound_of_float64(L, n_act, batch, k, m):
    """The bound: tests/drq_ref.py.  Samples whose branch (argmax, Huber side) the bound cannot pin are left out by the
    reference's own mask; it keeps at least 95 %."""
    worst, kept, total = 0., 0, 0
    for duel, dbl, wtd, clip in FLAGS:
        c = dr.drq_case(_seed(n_act, batch, duel, dbl, wtd, clip, k, m), n_act, batch, k, m, duel, dbl, wtd)
        dq, rows, td = _launch(L, c, GAMMA, clip)
        ref = dr.ref_drq64(c, GAMMA, clip)
        ok = ref["ok"]
        okv = np.tile(ok, m)
        kept, total = kept + int(ok.sum()), total + batch
        cols = n_act + int(duel)
        assert np.isfinite(dq).all() and np.isfinite(rows).all() and np.isfinite(td).all()
        for name, err, tol in (("dq", np.abs(dq[:, :cols] - ref["dq"]).max(axis=1)[okv], ref["dq_tol"][okv]),
                               ("loss_rows", np.abs(rows - ref["rows"])[ok], ref["rows_tol"][ok]),
                               ("td_abs", np.abs(td - ref["td"])[ok], ref["td_tol"][ok])):
            ratio = (err / np.maximum(tol, 1e-300)).max() if len(err) else 0.
            worst = max(worst, ratio)
            assert (err <= tol).all(), (name, duel, dbl, wtd, clip, ratio)
        _dq_is_zero_outside_the_taken_entries(c, dq)
    print("arl_drq_loss A%d B%d k%d m%d: largest error / bound %.3f; %d of %d samples kept" % (n_act, batch, k, m, worst, kept,
                                                                                            total))
    assert kept >= 0.95 * total


def test_loss_refusals_launch_nothing(L):
    lib = L.load()
    batch = 2
    big = torch.zeros(16 * batch, 260, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret = torch.zeros(batch, device=DEV)
    dq, rows, td = (torch.full(s, NAN, device=DEV) for s in ((16 * batch, 260), (batch,), (batch,)))
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def drq(q=p(big), nxt=p(big), acts=p(act), out=p(dq), r=p(rows), t=p(td), b=batch, m=2, k=2, a=6, s=8, duel=0):
        return lib.arl_drq_loss(q, nxt, None, acts, p(ret), p(act), None, b, m, k, a, s, duel, 0.99, 1.0, out, r, t, None)

    for kw in (dict(q=None), dict(nxt=None), dict(acts=None), dict(out=None), dict(r=None), dict(t=None)):
        assert drq(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(b=0), dict(a=0), dict(a=256, s=256), dict(s=10), dict(a=6, s=4), dict(a=8, s=8, duel=1),  # as arl_dqn_loss
               dict(m=0), dict(m=9), dict(k=0), dict(k=9), dict(b=2 ** 28, m=8, k=1), dict(b=2 ** 28, m=1, k=8)):
        assert drq(**kw) == E_RANGE, kw
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (dq, rows, td))
    assert drq(m=8, k=8, a=255, s=256) == 0 and drq(m=1, k=1, a=7, s=8, duel=1) == 0       # at the limits it runs
    torch.cuda.synchronize()
    assert torch.isfinite(dq.view(-1)[:8 * batch * 256]).all() and torch.isfinite(rows).all() and torch.isfinite(td).all()


# ---- policy ----------------------------------------------------------------------------------------------------------

N_ACT, BATCH = 6, 8


def _views(seed, m, k, adjacent=True):
    """m views of obs and k of next_obs for BATCH samples, view-major; adjacent: in one tensor, as the replay memory
    hands them out."""
    rs = np.random.RandomState(seed)
    both = _dev(rs.randint(0, 256, size=((m + k) * BATCH, 4, 104, 80), dtype=np.uint8))
    obs, nxt = (both[:m * BATCH], both[m * BATCH:]) if adjacent else (both[:m * BATCH].clone(), both[m * BATCH:].clone())
    return dict(obs=obs, nxt=nxt, act=_dev(rs.randint(0, N_ACT, size=BATCH).astype(np.uint8)),
                ret=_dev((rs.randn(BATCH) * 0.05).astype(np.float32)), term=_dev((rs.rand(BATCH) < 0.3).astype(np.uint8)),
                isw=_dev((rs.rand(BATCH) + 0.2).astype(np.float32)))


@pytest.mark.parametrize("adjacent", [True, False], ids=["adjacent", "apart"])
@pytest.mark.parametrize("double", [False, True], ids=["max", "double"])
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_policy_k_m_1_equals_q_loss_and_grads_bit_for_bit(dueling, double, adjacent):
    policy, _ = _make_policy("dqn", dueling=dueling)
    mb = _views(11, 1, 1, adjacent)
    args = (mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], GAMMA, 0.05)
    policy.flat_grads.fill_(NAN)
    rows, td = policy.q_loss_and_grads(*args, double_dqn=double)
    want = (policy.flat_grads.clone(), rows.clone(), td.clone())
    policy.flat_grads.fill_(NAN)
    rows, td = policy.drq_loss_and_grads(*args, double, 1, 1)
    assert rows.data_ptr() + 4 * BATCH == td.data_ptr()         # the (2, B) buffer the optimizer's ring takes at once
    assert torch.isfinite(want[0]).all() and want[0].abs().max() > 0
    for x, y in zip((policy.flat_grads, rows, td), want):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="rows"):
        policy.drq_loss_and_grads(*args, double, 2, 1)


@pytest.mark.parametrize("double", [False, True], ids=["max", "double"])
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_policy_k_m_2_matches_float64_autograd(dueling, double):
    """Tolerances: tests/test_dqn_gpu.py::test_training_step_matches_autograd_through_plain_torch's (rtol 2e-3, atol
    2e-5 max |grad|), on the float64 network of tests/test_munchausen_gpu.py (tests/autograd_ref.py holds the fp32
    policy-gradient network only) fed the same four views."""
    m = k = 2
    policy, spec = _make_policy("dqn", dueling=dueling)
    mb = _views(12, m, k)
    clip = 0.05
    target_before = policy.flat_target.clone()
    policy.flat_grads.fill_(NAN)
    rows, td = policy.drq_loss_and_grads(mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], GAMMA, clip,
                                         double, m, k)
    got = policy.bucket_to_reference(policy.flat_grads)
    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    scale = float(np.float32(1. / 255))
    obs, nxt = mb["obs"].cpu().double() * scale, mb["nxt"].cpu().double() * scale
    q = _ref_q(rp, spec, obs, dueling).view(m, BATCH, N_ACT)
    with torch.no_grad():
        tgt = _ref_q(rt, spec, nxt, dueling)
        sel = _ref_q(rp, spec, nxt, dueling) if double else tgt
        next_q = tgt[torch.arange(k * BATCH), sel.argmax(dim=1)].view(k, BATCH)
    ar, act = torch.arange(BATCH), mb["act"].cpu().long()
    y = mb["ret"].cpu().double() + (1. - mb["term"].cpu().double()) * GAMMA * next_q.mean(dim=0)
    d = y[None, :] - q[:, ar, act]
    ad = d.abs()
    loss_v = torch.where(ad <= clip, 0.5 * d * d, clip * (ad - clip / 2))
    want_rows = (mb["isw"].cpu().double() / BATCH / m) * loss_v.sum(dim=0)
    want_td = ad.clamp(max=clip).mean(dim=0)
    assert (ad < clip).any() and (ad > clip).any()              # both branches of the Huber loss in play
    want = np.concatenate([g.detach().numpy().reshape(-1) for g in torch.autograd.grad(want_rows.sum(), rp)])
    print("loss %.6g vs %.6g; max grad err %.3g of max |grad| %.3g" % (rows.sum().item(), want_rows.sum().item(),
                                                                       np.abs(got - want).max(), np.abs(want).max()))
    assert np.abs(want).max() > 0
    assert abs(rows.sum().item() - want_rows.sum().item()) <= 1e-4 * abs(want_rows.sum().item())
    assert torch.allclose(td.cpu().double(), want_td, rtol=2e-3, atol=1e-6)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    assert torch.equal(policy.flat_target, target_before)       # the target network is read, never written


# ---- algorithms ------------------------------------------------------------------------------------------------------

def _train_drq(prioritized, use_graph):
    from accel_rl_amd.algos.dqn.drq import DrQ
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecEvalSampler(eval_steps=8 * 20, eval_envs_per=1, EnvCls=SynthAtariEnv, env_args=dict(game="seaquest"),
                                horizon=4, n_parallel=4, envs_per=2, max_path_length=25, max_decorrelation_steps=0,
                                device=DEV)
    algo = DrQ(k_targets=2, m_online=2, aug_seed=3, batch_size=BATCH, min_steps_learn=64 * 4, replay_size=64 * 40,
               training_intensity=0.5, target_update_steps=64 * 2, reward_horizon=3, prioritized_replay=prioritized,
               eps_greedy_args=dict(anneal_steps=64 * 6), optimizer_args=dict(use_graph=use_graph))
    policy = AtariDqnPolicy(dueling=True, **dict(cnn_specs[0], hidden_sizes=[64]))
    first = {}
    initialize = policy.initialize

    def recording_initialize(*a, **kw):
        initialize(*a, **kw)
        first["params"] = policy.get_param_values()
    policy.initialize = recording_initialize
    runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 10, seed=9, eval_interval_steps=64 * 5)
    runner.train()
    return algo, policy, first["params"], runner.last_tabular


@pytest.mark.parametrize("prioritized", [True, False], ids=["prioritized", "uniform"])
def test_drq_trains_and_replayed_updates_equal_eager_ones(prioritized):
    """DrQ (K = M = 2) through the runner on the synthetic environment, 64 steps and 4 updates per iteration: the third
    update is captured and every later one replayed; the same seeded run with eager updates ends in the same parameters
    bit for bit (there is no generator inside the graph: the shifts are drawn by the eager extraction, from the host's
    call counter)."""
    algo, policy, first, tab = _train_drq(prioritized, True)
    assert algo.optimizer._graph is not None and algo._updates_per_optimize == 4
    assert algo.replay_buffer._augment["call"] >= 4 * 6 and algo.replay_buffer._augment["m_obs"] == 2
    mb_obs, mb_next = algo.replay_buffer._batch_outputs(BATCH)[:2]
    assert mb_obs.shape[0] == 2 * BATCH and mb_next.data_ptr() == mb_obs.data_ptr() + mb_obs.numel()
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, first)
    assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["PriorityAverage"] > 0
    target = policy.bucket_to_reference(policy.flat_target)
    assert np.isfinite(target).all() and not np.array_equal(target, first)
    algo_e, policy_e, first_e, _ = _train_drq(prioritized, False)
    assert algo_e.optimizer._graph is None and np.array_equal(first, first_e)
    assert algo_e.replay_buffer._augment["call"] == algo.replay_buffer._augment["call"]
    np.testing.assert_array_equal(policy_e.get_param_values(), final)


@pytest.mark.parametrize("kind", ["qr", "fqf"])
def test_the_family_inherits_augmented_replay(kind):
    """QuantileDQN / FQF with augment_args: two updates on a hand-filled replay memory; the minibatch the loss read is
    the shifted extraction of the sampled indices (drq_ref.shifted_extract), and differs from their plain extraction."""
    from accel_rl_amd.algos.dqn.fqf import FQF
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(4)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = (AtariFqfPolicy if kind == "fqf" else AtariQrDqnPolicy)(epsilon=0.3, n_quantiles=8, **spec)
    env_spec = EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT))
    policy.initialize(env_spec, device=DEV)
    algo = (FQF if kind == "fqf" else QuantileDQN)(batch_size=BATCH, min_steps_learn=0, replay_size=64, training_intensity=2,
                                                  augment_args=dict(pad=4, seed=21))
    n_env, horizon = 2, 4
    algo.initialize(policy, env_spec, n_env * horizon, horizon, True)
    rb = algo.replay_buffer
    assert rb._augment == dict(pad=4, seed=21, m_obs=1, k_next=1, call=0) and algo._updates_per_optimize == 2
    rs = np.random.RandomState(8)

    def samples():
        n = n_env * horizon
        return dict(observations=_dev(rs.randint(0, 256, (n, 4, 104, 80), dtype=np.uint8)),
                    actions=_dev(rs.randint(0, N_ACT, n).astype(np.uint8)), rewards=_dev(rs.randn(n).astype(np.float32)),
                    dones=_dev((rs.rand(n) < 0.1).astype(np.uint8)))
    for _ in range(3):
        rb.append_data(samples())
    drawn = []
    extract = rb.extract_batch

    def recording_extract(env_idxs, step_idxs):
        drawn.append((np.array(env_idxs), np.array(step_idxs), rb._augment["call"]))
        return extract(env_idxs, step_idxs)
    rb.extract_batch = recording_extract
    before = policy.get_param_values()
    minibatch, info = algo.optimize_policy(3, samples())
    torch.cuda.synchronize()
    assert len(drawn) == 2 and rb._augment["call"] == 2 and len(info["Loss"]) == 2
    after = policy.get_param_values()
    assert np.isfinite(after).all() and not np.array_equal(after, before)
    env, step, call = drawn[-1]
    got_obs, got_next = minibatch[0].cpu().numpy(), minibatch[1].cpu().numpy()
    rb.extract_batch = extract
    plain = rb.extract_observations(env, step).cpu().numpy()
    assert rb._augment["call"] == 2                             # an unshifted read draws nothing
    store = dict(frames=rb.frames.cpu().numpy().reshape(n_env, -1, 104 * 80), n_blanks=rb.n_blanks.cpu().numpy(),
                 acts=rb.acts.cpu().numpy(), returns=rb.returns.cpu().numpy(), terminals=rb.terminals.cpu().numpy())
    want = dr.shifted_extract(store, rb.env_replay_size, 4, 1, 104, 80, env, step, 4, 1, 1, 21, call)
    np.testing.assert_array_equal(got_obs, want[0])
    np.testing.assert_array_equal(got_next, want[1])
    unshifted = dr.shifted_extract(store, rb.env_replay_size, 4, 1, 104, 80, env, step, 0, 1, 1, 21, call)[0]
    np.testing.assert_array_equal(plain, unshifted)
    assert not np.array_equal(got_obs, plain)
