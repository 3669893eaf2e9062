"""CPU half of the R2D2 / V-MPO / SAC-Discrete limits tests (the device half is
tests/test_r2d2_vmpo_sacd_limits_gpu.py): every constructed case contains what it claims.

- the sequence layer: SeqModel -- the yardstick, unchanged -- writes exactly horizon / S state slots per environment at
  every idx, other slots than at idx = 0 for some idx, and the shapes of the device half take the loop trips and the
  t0 != 0 branch they were chosen for (arithmetic on the kernel's loop bounds as csrc/r2d2.hip states them);
- the R2D2 loss cases hold their plants at every configuration the device half runs;
- the V-MPO cases built from keys: vmpo_ref.select equals a plain sort on (key descending, position ascending), the pass
  that first decides, the bin that holds the threshold, its place in its lane and the two edge counts are what the
  case's name says, computed here from the keys alone;
- SAC-Discrete: rows of every kind lie in a second or later workgroup, and the stated summation order of
  arl_sacd_alpha_grad differs from a plain ascending sum -- and from the fold without its last step -- in some bit."""
import numpy as np
import pytest

import r2d2_ref as rr
import sacd_ref as sr
import vmpo_ref as vr

# ---- the sequence layer ----------------------------------------------------------------------------------------------------

BIG = dict(n_env=2, horizon=520, size=1040, S=4, hidden=1024)   # the device half's large store shape
BIG_IDX = [0, 3, 1037]
SMALL = dict(size=40, S=8, horizon=16)


def test_seq_model_writes_horizon_over_s_slots_at_every_idx():
    size, S, horizon = SMALL["size"], SMALL["S"], SMALL["horizon"]
    at_zero = rr.seq_written_slots(size, S, horizon, 0)
    assert at_zero == {0, 1}
    differing, t0s = 0, set()
    for idx in range(size):
        slots = rr.seq_written_slots(size, S, horizon, idx)
        assert len(slots) == horizon // S, idx
        first = (idx + rr.seq_t0(S, idx)) % size
        assert slots == {((first + k * S) % size) // S for k in range(horizon // S)}, idx
        differing += slots != at_zero
        t0s.add(rr.seq_t0(S, idx))
    assert differing >= size - S and t0s == set(range(S))       # every t0 the stride allows
    for idx in BIG_IDX:
        slots = rr.seq_written_slots(BIG["size"], BIG["S"], BIG["horizon"], idx)
        assert len(slots) == BIG["horizon"] // BIG["S"] == 130
    assert [rr.seq_t0(4, i) for i in BIG_IDX] == [0, 1, 3]
    assert 1037 + BIG["horizon"] > BIG["size"] and 0 in rr.seq_written_slots(1040, 4, 520, 1037)    # the batch wraps
    # the extremes: a full lap from a non-zero idx, S = 1, S = horizon = size
    assert rr.seq_written_slots(24, 4, 24, 5) == set(range(6))
    assert rr.seq_written_slots(12, 1, 6, 9) == {9, 10, 11, 0, 1, 2}
    assert rr.seq_written_slots(16, 16, 16, 7) == {0} and rr.seq_t0(16, 7) == 9


def test_seq_shapes_take_the_loop_trips_they_were_chosen_for():
    trips = lambda count: -(-count // 256)                                                # noqa: E731
    assert trips(BIG["horizon"]) == 3                                                     # the reset loop
    per = (BIG["horizon"] // BIG["S"]) * (BIG["hidden"] // 4)
    assert per == 130 * 256 and trips(per) == 130                                         # the state-copy loop
    assert trips(8) == 1 and trips((8 // 2) * (64 // 4)) == 1                             # (test_r2d2_gpu.py: one trip each)
    assert trips(600) == 3 and trips(11) == 1                                             # prepare's loop over t
    assert 100 > 2 * 40                                                                   # U = 100 laps a ring of 40 twice
    assert 1024 // 4 == 256 and trips(1024 // 4) == 1 and trips(1024 // 4 + 1) == 2       # hidden = 1024: the last full trip


# ---- arl_r2d2_loss ---------------------------------------------------------------------------------------------------------

def loss_configs():
    """(eps, weighted, eta, gamma_n or None for the shape's own)"""
    out = [(eps, w, eta, None) for eps in (1e-3, 0.0) for w in (True, False) for eta in (0.0, 1.0, 0.9)]
    return out + [(1e-3, True, 0.9, 0.0)]


@pytest.mark.parametrize("shape", rr.LIMIT_SHAPES[:4], ids=str)
def test_limit_loss_cases_contain_their_plants(shape):
    batch, burn_in, train_len, n, n_act, stride, duel = shape
    U = burn_in + train_len + n
    gamma = 0.997 ** n
    c = rr.limits_loss_case(10 * batch + n_act, *shape, gamma_n=gamma)
    first, last = burn_in, burn_in + train_len - 1
    assert c["terminals"][first] and c["terminals"][last]
    assert c["actions"][batch * U - n - 1] == 255 and n_act <= 255
    assert (c["q"][:, n_act + duel:] == rr.PAD).all() and (c["q_tgt"][:, n_act + duel:] == rr.PAD).all()
    if duel and stride == n_act + 1:
        assert (n_act % 4) == 3                                  # the value column is the last float of a float4
    for eps, weighted, eta, g in loss_configs():
        want = rr.r2d2_loss64(c["q"], c["q_tgt"], c["actions"], c["returns"], c["terminals"],
                              c["is_weights"] if weighted else None, batch, burn_in, train_len, n, n_act, bool(duel),
                              gamma if g is None else g, eps, eta)
        assert (want["x"] == 0).any() and (want["z"] == 0).any() and want["a_star"][0, 0] == 0
        ad = np.abs(want["d"])
        assert ad[0].argmax() == train_len - 1                   # the largest |d| of sequence 0 is its last
        if train_len > 1:
            assert ad[0, -1] > 1.5 * ad[0, :-1].max()
            # a walk that stopped one entry short, or at 512, would give other float32 values
            short = 0.5 * (want["d"][0, :-1] ** 2).sum()
            assert np.float32(short) != np.float32(0.5 * (want["d"][0] ** 2).sum())
        for key in ("dq", "td_abs", "loss_rows", "priorities"):
            assert np.isfinite(want[key]).all()
    if n_act > 200:
        act = np.minimum(c["actions"].astype(np.int64), n_act - 1)
        assert act[batch * U - n - 1] == n_act - 1 == 254        # the byte 255 reads as 254
    if batch >= 2:
        assert np.abs(c["q"][U:2 * U, :n_act]).max() > 5e3


def test_limit_loss_shapes_reach_the_kernel_s_limits():
    s0, s1, s2, s3, s4 = rr.LIMIT_SHAPES
    assert s0[1] == 1024 and s0[2] == 1024 and s0[3] == 16 and s0[5] == s0[4] + 1
    U0 = s0[1] + s0[2] + s0[3]
    assert U0 * s0[5] // 4 == 2064 and 2064 % 64 != 0            # the dq writer's last pass is ragged
    assert s1[2] == 1023 and 1023 // 64 == 15 and 1023 % 64 == 63 and s1[5] == s1[4] + 1 == 256
    assert s2[4] == 255 and not s2[6] and s3[1] == 1024 and s3[2] == 1
    assert s4[0] - 1 > 65535


# ---- arl_vmpo_weights ------------------------------------------------------------------------------------------------------

def _plain_selection(k):
    order = np.lexsort((np.arange(k.size), -k.astype(np.int64)))          # key descending, then position ascending
    sel = np.zeros(k.size, bool)
    sel[order[:(k.size + 1) // 2]] = True
    return sel


@pytest.mark.parametrize("n", vr.LIMIT_SIZES)
def test_radix_cases_decide_in_the_pass_and_bin_they_name(n):
    lanes_r = set()
    for name, p, T, edge in vr.radix_families(n):
        k = vr.radix_case(np.random.RandomState(1000 * p + T + n), n, p, T, edge)
        adv = vr.from_keys(k)
        assert k.size == n and np.array_equal(vr.select(adv), _plain_selection(k)), name
        trace, thr, left = vr.radix_trace(k)
        assert thr == int(np.sort(k)[::-1][(n + 1) // 2 - 1]), name                       # the n_top-th largest key
        assert left == (n + 1) // 2 - int((k > thr).sum()) and left >= 1, name
        t = trace[p]
        assert t["bin"] == T and t["lane"] == (255 - T) // 4 and t["r"] == (255 - 4 * t["lane"]) - T, name
        assert all(trace[q]["bins"] == 1 and trace[q]["want"] == (n + 1) // 2 for q in range(p)), name
        if n > 1:
            assert vr.first_deciding_pass(trace) == p and t["candidates"] == n, name
        if edge == "incl":
            assert t["want"] == t["incl"] and (n == 1 or t["incl"] < n), name
        if edge == "above1":
            assert t["want"] == t["above"] + 1 and (n == 1 or t["above"] >= 1), name
            assert sum(t["c"][:t["r"]]) == 0, name
        if edge == "mid" and n >= 1025:
            assert t["above"] + 1 < t["want"] < t["incl"] or T in (0, 255), name
            assert min(t["c"]) > 0, name                                                  # all four of the lane's bins filled
        lanes_r.add((p, t["lane"], t["r"]))
    for p in range(4):                                          # each of the nested c0 .. c3 branches, both end lanes
        assert {(p, vr.LANE_OF_PASS[p], r) for r in range(4)} <= lanes_r
        assert (p, 0, 0) in lanes_r and (p, 63, 3) in lanes_r


@pytest.mark.parametrize("n", vr.LIMIT_SIZES)
def test_sign_and_range_cases_hold_what_they_name(n):
    cases = dict((name, (adv, eta)) for name, adv, eta in vr.sign_and_range_cases(np.random.RandomState(n), n))
    n_top = (n + 1) // 2
    for name, (adv, eta) in cases.items():
        k = vr.keys(adv)
        assert adv.dtype == np.float32 and adv.size == n and np.isfinite(adv).all(), name
        assert np.array_equal(vr.select(adv), _plain_selection(k)), name
        assert np.float32(eta) > 0, name                         # (vmpo_ref.weights rounds eta to fp32, as the device holds it)
    k = vr.keys(cases["all-negative"][0])
    assert (cases["all-negative"][0] < 0).all() and (k < 0x80000000).all()                # the inverted half alone
    trace, thr, _ = vr.radix_trace(vr.keys(cases["threshold-is-plus-zero"][0]))
    assert thr == 0x80000000 and trace[0]["bin"] == 128 and trace[0]["r"] == 3
    if n > 1:
        assert (vr.keys(cases["threshold-is-plus-zero"][0]) == 0x7FFFFFFF).sum() == 1     # its neighbour is not selected
        assert trace[0]["want"] == trace[0]["incl"] == n_top
    trace, thr, _ = vr.radix_trace(vr.keys(cases["threshold-is-minus-zero"][0]))
    assert thr == 0x7FFFFFFF and trace[0]["bin"] == 127 and trace[0]["r"] == 0
    assert trace[0]["want"] == trace[0]["above"] + 1 == n_top
    den = cases["denormals-eta1"][0]
    assert (np.abs(den) < 2.0 ** -126).all() and (den != 0).all()
    assert n < 3 or ((den > 0).any() and (den < 0).any())
    assert cases["denormals-eta-min"][1] == 2.0 ** -126
    if n >= 1025:                                               # at the smallest eta the denormals' weights differ
        ref = vr.weights(den, 2.0 ** -126, 0.01)
        assert ref["psi"][ref["sel"]].max() > 1.5 * ref["psi"][ref["sel"]].min()
        assert abs(ref["temp_loss"]) < 2.0 ** -126              # and the dual loss is itself a denormal fp32 number
    big = cases["near-flt-max-eta1"][0]
    fmax = float(np.finfo(np.float32).max)
    assert np.abs(big).max() <= 0.9 * fmax and (n < 1025 or np.abs(big).max() > 0.85 * fmax)


def test_from_keys_refuses_keys_of_values_that_are_not_finite():
    for bad in (0x007FFFFF, 0xFF800000, 0x00000000, 0xFFFFFFFF):
        with pytest.raises(AssertionError):
            vr.from_keys(np.array([bad], np.uint32))
    edge = vr.from_keys(np.array([vr.KEY_MIN, vr.KEY_MAX, 0x80000000, 0x7FFFFFFF], np.uint32))
    fmax = np.finfo(np.float32).max
    assert edge[0] == -fmax and edge[1] == fmax and edge[2] == 0 and not np.signbit(edge[2]) and np.signbit(edge[3])


# ---- SAC-Discrete ----------------------------------------------------------------------------------------------------------

def test_sacd_limit_cases_put_every_kind_of_row_in_a_later_workgroup():
    seen = set()
    for shape in sr.LIMIT_SHAPES:
        n_act, stride, batch, shift = shape
        for weighted in (False, True):
            c = sr.limit_case(shape, weighted)
            later = set(c["kinds"][256:].tolist())
            seen |= later
            if batch >= 513:
                assert later == set(range(sr.N_KINDS)), shape
                assert set(c["kinds"][batch - batch % 256:].tolist()) <= later            # the one-row tail block
            assert (c["q1"][:, n_act:] == sr.POISON).all() and c["q1"].shape == (batch, stride)
            assert ((c["act"] == 255) == (c["kinds"] == sr.ACT_OUTSIDE)).all()
            ref = sr.ref_loss(c, sr.GAMMA, 1.0)
            assert all(np.isfinite(ref[key]).all() for key in ("dq1", "dlogits", "rows", "td", "ent", "pi_rows"))
    assert seen == set(range(sr.N_KINDS))
    c = sr.limit_case(sr.LIMIT_SHAPES[1], True)
    assert c["kinds"][256] == sr.ACT_OUTSIDE and c["act"][256] == 255                     # row 256 of 257, A = 253


@pytest.mark.parametrize("batch", sr.ALPHA_GRAD_BATCHES)
def test_alpha_grad_restatement_tells_its_order_from_the_plain_sum(batch):
    ent = sr.alpha_grad_rows(batch)
    own = sr.alpha_grad_sum32(ent)
    assert own.dtype == np.float32
    exact = float(ent.astype(np.float64).sum())
    assert abs(float(own) - exact) <= (batch / 256. + 9) * sr.EPS * exact                 # (a sum of positive numbers)
    if batch == 1:
        assert own == ent[0] == sr.plain_sum32(ent)
        return
    bits = lambda x: np.float32(x).view(np.uint32)                                        # noqa: E731
    assert bits(own) != bits(sr.plain_sum32(ent))
    assert bits(own) != bits(sr.alpha_grad_sum32(ent, drop_last_fold=True))
    g = sr.alpha_grad32(ent, sr.ALPHA_GRAD_TARGET)
    assert g.dtype == np.float32
    assert bits(g) != bits(np.float32(sr.plain_sum32(ent) / np.float32(batch)) - sr.ALPHA_GRAD_TARGET)
    want, atol = sr.ref_alpha_grad(ent, np.float32(0.0), float(sr.ALPHA_GRAD_TARGET))
    assert abs(float(g) - want) <= atol
