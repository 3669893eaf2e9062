"""What tests/test_quantile_limits_gpu.py relies on, proved on the CPU: that every named case reaches the branch it names,
that the fp32 restatement of tests/quantile_ref.py stays inside the project's existing bounds of the float64 references,
that the chosen inputs tell the header's summation orders from other orders (otherwise bit-equality would prove nothing
about order), and the cosine exactness claim of include/accel_rl_hip.h (arl_iqn_embed).

The exactness claim.  |tau| = s 2^e with s its 24-bit significand; the angle i tau, the period 2 and the fold points 1
and 1/2 are all multiples of 2^e once e <= -1, so the folded t is m 2^e with an integer m, and t <= 1/4 gives
m <= 2^(-2 - e).  m has at most 24 significant bits for every i and s exactly when -2 - e <= 24, i.e. e >= -26, i.e.
|tau| >= 2^-3: the test finds that binade by trying them, exhaustively over the 2^23 significands for a few i (the
counter-example's i = 21 among them) and on a random sample for every i, and asserts the counter-examples below it
(2^-5 (1 + 2^-23) at i = 21: 26 bits; 2^-4 (1 + 2^-23): 25).  A drawn fraction is (2 k + 1) 2^-24: m <= 2^22."""
import numpy as np
import pytest
import torch

import fqf_ref as fr
import munchausen_ref as mr
import quantile_ref as qr
from quantile_ref import F32
from test_iqn_gpu import _check_against, _reference, ref_tau

GAMMA = float(np.float32(0.99 ** 3))
KAPPAS = (0.0, 0.25, 1.0)
N_TARGETS = (1, 2, 3, 4, 5, 63, 64)


def _bits_of(x):
    return int(qr.bits(np.array([x], F32))[0])


# ---- the cosine reduction ---------------------------------------------------------------------------------------------------

def test_every_branch_of_the_cosine_reduction_is_named_by_a_case():
    want = {"one": [(0, 0.3), (5, 0.0), (5, 2.0 ** 24), (5, float("inf")), (5, float("nan")), (3, -2.0 ** 25)],
            "unreduced": [(1, 2.0 ** -15), (63, 2.0 ** -24), (63, 1e-45), (1, np.nextafter(F32(2.0 ** -14), F32(0)))],
            "none": [(1, 2.0 ** -14), (1, 0.25), (1, 0.1)],
            "sin": [(1, 0.3), (1, 0.5)],
            "pi": [(1, 0.8), (1, 1.0)],
            "pi+sin": [(1, 0.7)],
            "2pi": [(1, 1.9)],
            "2pi+sin": [(1, 1.6)],
            "2pi+pi": [(1, 1.2)],
            "2pi+pi+sin": [(1, 1.3)]}
    for name, cases in want.items():
        for i, tau in cases:
            assert qr.cos_branch(i, _bits_of(tau)) == name, (name, i, tau)
    # both sides of sh == 40: the significand's exponent e = -38 is |tau| in [2^-15, 2^-14), e = -37 is [2^-14, 2^-13)
    assert qr.cos_reduce(1, _bits_of(np.nextafter(F32(2.0 ** -14), F32(0))))[1] == 40
    assert qr.cos_reduce(1, _bits_of(2.0 ** -14))[1] == 39
    # exact values the header states
    assert qr.cos_f64(1, _bits_of(0.5)) == 0.0 and qr.cos_f64(3, _bits_of(-0.5)) == 0.0 and qr.cos_f64(2, _bits_of(0.75)) == 0.0
    assert qr.cos_f64(1, _bits_of(1.0)) == -1.0 and qr.cos_f64(7, _bits_of(2.0)) == 1.0 and qr.cos_f64(1, _bits_of(3.0)) == -1.0


def test_the_given_grid_reaches_every_branch_and_the_short_butterfly_is_the_long_one():
    given = qr.tau_grid()
    assert {qr.cos_branch(i, w) for w in qr.bits(given) for i in (1, 21, 63)} == qr.COS_BRANCHES
    assert (qr.bits(given) >> 23 & 0xff == 0).sum() >= 12 and np.isnan(given).any() and np.isinf(given).sum() == 2
    rs = np.random.RandomState(9)
    for n in (1, 2, 3, 5, 31, 32, 33, 63, 64):
        x = (rs.randn(50, n) * 3).astype(F32)
        x[0] = -0.0
        x[1, ::2] = 0
        np.testing.assert_array_equal(qr.bits(qr.wave_sum(x)), qr.bits(qr.wave_sum_64(x)))


def test_the_integer_reduction_agrees_with_float64_and_ignores_the_sign():
    rs = np.random.RandomState(0)
    tau = np.concatenate([rs.uniform(0, 1, 200), rs.uniform(-40, 40, 100), 2.0 ** rs.uniform(-30, 23, 100)]).astype(F32)
    got = qr.cos_f64_table(tau)
    want = np.cos(np.pi * np.fmod(np.arange(64.)[None, :] * tau.astype(np.float64)[:, None], 2.0))
    assert np.abs(got - want).max() <= 1e-15 * 64 * 40          # (float64's own pi i tau rounding at |i tau| <= 2520)
    np.testing.assert_array_equal(got, qr.cos_f64_table(-tau))


def _max_bits(binade, i_values, significands):
    """The largest number of significant bits of the folded argument over `significands` (24-bit, uint64) in the binade
    [2^binade, 2^(binade + 1)) and the feature indices i_values."""
    sh = 2 - (binade - 23)
    return max(int(qr.significant_bits_vec(i, significands, sh).max()) for i in i_values)


def test_the_folded_argument_converts_exactly_from_the_binade_of_one_eighth():
    every = np.arange(2 ** 23, 2 ** 24, dtype=np.uint64)
    sample = np.unique(np.concatenate([np.random.RandomState(1).randint(2 ** 23, 2 ** 24, size=1 << 16).astype(np.uint64),
                                       np.array([2 ** 23, 2 ** 23 + 1, 2 ** 24 - 1], np.uint64)]))
    exhaustive_i = (21, 43, 63)
    worst = {}
    for binade in range(-8, 1):                                 # [2^-8, 2^-7) ... [1, 2): a given tau may exceed 1
        worst[binade] = max(_max_bits(binade, exhaustive_i, every if binade in (-4, -3, -2) else sample),
                            _max_bits(binade, range(1, 64), sample))
    print("largest significant-bit count of t per binade:", worst)
    smallest_exact = min(b for b in worst if all(worst[c] <= 24 for c in worst if c >= b))
    assert smallest_exact == -3, worst
    assert worst[-4] == 25 and worst[-5] == 26                  # the lsb argument's 2^(-2 - e), reached
    # the counter-examples, through the scalar restatement
    for binade, bits_ in ((-5, 26), (-4, 25), (-3, 24)):
        tau = F32(2.0 ** binade * (1 + 2.0 ** -23))
        assert max(qr.significant_bits(qr.cos_reduce(i, _bits_of(tau))[0]) for i in range(1, 64)) == bits_, binade
    assert qr.significant_bits(qr.cos_reduce(21, _bits_of(F32(2.0 ** -5 * (1 + 2.0 ** -23))))[0]) == 26
    # above [1, 2) the lsb only grows; at and above 2^23 tau is an integer and t is 0 (or the reduction returns early)
    for binade in (1, 5, 12, 22):
        assert _max_bits(binade, range(1, 64), sample) <= 24
    # a drawn fraction is (2 k + 1) 2^-24 whatever its binade: at most 22 bits
    drawn = ref_tau(7, 3, np.arange(4096))
    assert max(qr.significant_bits(qr.cos_reduce(i, w)[0]) for w in qr.bits(drawn)[:256] for i in range(1, 64)) <= 22
    # vector and scalar restatements agree
    for s in (2 ** 23 + 1, 2 ** 24 - 1, 0xC90FDB):
        for i in (1, 21, 63):
            w = ((127 - 4) << 23) | (s & 0x7fffff)
            assert qr.significant_bits(qr.cos_reduce(i, w)[0]) == int(qr.significant_bits_vec(i, np.array([s], np.uint64), 29)[0])


# ---- the loss corners --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kappa", KAPPAS)
def test_corner_rows_reach_the_branches_they_name(kappa):
    n_act, n, m, stride = 64, 64, 5, 64
    c = qr.corner_case(3, n_act, n, m, stride, kappa)
    out = qr.iqn_loss(c["pred"], c["tau"], c["tgt"], c["pol"], c["act"], c["ret"], c["term"], c["isw"], n_act, GAMMA, kappa)
    np.testing.assert_array_equal(out["a_next"], c["chosen"])
    q = qr.q_of_lane(c["pol"], n_act)
    assert q[qr.ROW_TIE, 0] == q[qr.ROW_TIE, n_act - 1] == q[qr.ROW_TIE].max() and out["a_next"][qr.ROW_TIE] == 0
    assert out["a_next"][qr.ROW_LAST_LANE] == 63
    assert c["act"][qr.ROW_ACTION_255] == 255 and out["dtheta"][qr.ROW_ACTION_255, :, n_act - 1].any()   # an act >= A row
    assert set(c["act"].tolist()) >= {0, n_act - 1}
    u = out["T"][qr.ROW_KAPPA_EDGES][None, :] - c["pred"][qr.ROW_KAPPA_EDGES, :, 0][:, None]
    k = F32(kappa)
    assert (u == 0).any()                                       # exact u == 0: counts as not negative
    if kappa > 0:
        for sign in (1, -1):
            for v in (k, np.nextafter(k, F32(0)), np.nextafter(k, F32(np.inf))):
                assert (u == F32(sign) * v).any(), (sign, v)
    assert out["loss_b"][qr.ROW_TINY_LOSS] < 1e-6 and out["pri"][qr.ROW_TINY_LOSS] == F32(1e-6)       # both priority clamps
    assert out["loss_b"][qr.ROW_HUGE_LOSS] > 1e6 and out["pri"][qr.ROW_HUGE_LOSS] == F32(1e6)
    assert out["rows"][qr.ROW_ZERO_WEIGHT] == 0 and not out["dtheta"][qr.ROW_ZERO_WEIGHT].any()
    assert c["tau"][qr.ROW_TAU_ENDS, 0] == 0 and c["tau"][qr.ROW_TAU_ENDS, -1] == 1
    assert c["term"][qr.ROW_TERMINAL] == 1 and c["term"][qr.ROW_PLAIN] == 0


@pytest.mark.parametrize("m", N_TARGETS)
def test_small_target_counts_leave_waves_without_a_term(m):
    T = np.ones((1, m), F32)
    g, r = qr.strided_partials(T, np.zeros((1, 3), F32), np.full((1, 3), 0.5, F32), 1.0)
    for w in range(4):
        assert bool(g[w].any()) == (w < m) and bool(r[w].any()) == (w < m)     # N' below 4: waves N' .. 3 get no j
    counts = [len(range(w, m, 4)) for w in range(4)]
    assert sum(counts) == m and (m % 4 == 0) == (len(set(counts)) == 1)


def _as_got(out, n_act):
    return torch.from_numpy(out["dtheta"]), torch.from_numpy(out["rows"]), torch.from_numpy(out["pri"])


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n,m", [(1, 1), (64, 5), (63, 64), (64, 63), (1, 4), (63, 3), (64, 2)])
def test_the_fp32_restatement_is_inside_the_float64_bounds_of_the_feature_tests(n, m, kappa):
    n_act, stride = 64, 68
    c = qr.corner_case(100 * n + m, n_act, n, m, stride, kappa)
    out = qr.iqn_loss(c["pred"], c["tau"], c["tgt"], c["pol"], c["act"], c["ret"], c["term"], c["isw"], n_act, GAMMA, kappa)
    c64 = dict(c, act=qr.clamp_action(c["act"], n_act).astype(np.uint8))    # the float64 reference indexes: clamp first
    ref = _reference(c64, n_act, GAMMA, kappa)                  # (identical columns sum identically in float64 too, and
    assert ref["margin"] == 0                                   # torch.argmax returns the first maximum: the tie row)
    q64 = torch.from_numpy(c["pol"][:, :, :n_act].astype(np.float64)).sum(dim=1) / m
    q64[qr.ROW_TIE, n_act - 1] = -1e9
    top2 = torch.topk(q64, 2, dim=1).values
    ref["margin"] = (top2[:, 0] - top2[:, 1]).min().item()      # every other margin: at least 20 - a few sigma
    _check_against(ref, _as_got(out, n_act), c64, n_act, kappa if kappa > 0 else None, exact_u=kappa == 0)


def test_another_order_changes_a_bit_on_the_chosen_inputs():
    """The three orders the header could be mistaken for, on the corner cases the GPU test runs bit for bit."""
    changed = dict(ascending=0, pairs=0, sequential=0)
    total = 0
    for kappa in KAPPAS:
        for n, m in ((64, 64), (63, 5), (64, 63)):
            c = qr.corner_case(100 * n + m, 64, n, m, 64, kappa)
            out = qr.iqn_loss(c["pred"], c["tau"], c["tgt"], c["pol"], c["act"], c["ret"], c["term"], c["isw"], 64, GAMMA, kappa)
            act = qr.clamp_action(c["act"], 64)
            batch = c["pred"].shape[0]
            th = c["pred"][np.arange(batch), :, act]
            wgt = qr.weights(c["isw"], batch)
            g, r = qr.strided_partials(out["T"], th, c["tau"], kappa)
            ga, ra = qr.ascending_j_sums(out["T"], th, c["tau"], kappa)
            d_asc = -(wgt[:, None] / F32(m) * ga)
            d_pairs, rows_pairs, _, _ = qr.reduce_tail(out["T"], th, c["tau"], wgt, kappa, combine=qr.combine4_pairs)
            _, rows_seq, _, _ = qr.reduce_tail(out["T"], th, c["tau"], wgt, kappa, total=qr.sequential_sum)
            total += 1
            changed["ascending"] += int((qr.bits(d_asc) != qr.bits(out["d"])).any())
            changed["pairs"] += int((qr.bits(d_pairs) != qr.bits(out["d"])).any() or (qr.bits(rows_pairs) != qr.bits(out["rows"])).any())
            changed["sequential"] += int((qr.bits(rows_seq) != qr.bits(out["rows"])).any())
    print("cases (of %d) in which the other order changes a bit:" % total, changed)
    assert all(v >= 1 for v in changed.values()), changed
    # QR-DQN's Q and FQF's entropy: the butterfly against a sequential sum
    rs = np.random.RandomState(5)
    theta = (rs.randn(8, 65, 64) * 2).astype(F32)
    assert (qr.bits(qr.qr_q(theta, 64, 64, True)) !=
            qr.bits(qr.sequential_sum(qr.qr_merged(theta, 64, 64, True)) / F32(64))).any()
    # FQF: S_k with i == k included
    g = (rs.randn(4, 64)).astype(F32)
    g[:, 0] = 0
    part = qr.fqf_fraction_part(np.zeros((4, 64), F32), np.zeros((4, 63), F32), np.zeros((4, 65), F32), np.ones((4, 64), F32),
                                np.zeros((4, 64), F32), np.zeros(4, F32), np.ones(4, F32), 0., 64)
    assert not part["S"].any()
    assert (qr.fqf_suffix_including_k(g)[:, 1:] != 0).any()


@pytest.mark.parametrize("k", [3, 5, 63, 64])
def test_order_sensitive_action_values_tell_ascending_from_descending(k):
    theta = qr.order_sensitive_theta(k, k, 3)
    up, down = qr.first_max(qr.q_of_lane(theta, 3)), qr.first_max(qr.q_of_lane_descending(theta, 3))
    assert (up != down).all() and set(up.tolist()) | set(down.tolist()) == {0, 2}
    lg = np.zeros((1, k), F32)
    lg[0] = (np.random.RandomState(k).randn(k) * 0.5).astype(F32)
    tau = _host_fractions(lg, k)["tau"][0]
    theta = qr.order_sensitive_theta(k, k, 3, tau=tau)
    t = np.ascontiguousarray(np.broadcast_to(tau, (theta.shape[0], k + 1)))
    assert (qr.first_max(qr.wq_of_lane(theta, t, 3)) != qr.first_max(qr.wq_of_lane_descending(theta, t, 3))).all()


# ---- QR-DQN ------------------------------------------------------------------------------------------------------------------

def test_qrdqn_restatement_against_float64_and_its_dueling_rows():
    from test_qrdqn_gpu import ref_qr_loss                      # float64
    rs = np.random.RandomState(2)
    for n_act, n, stride, dueling in ((64, 64, 64, True), (63, 2, 4, True), (2, 2, 4, False)):
        batch = 4
        rows = n_act + int(dueling)
        pred, tgt = ((rs.randn(batch, rows, stride) * 2).astype(F32) for _ in range(2))
        pred[:, :, n:], tgt[:, :, n:] = qr.POISON, qr.POISON
        tgt[:, 1 % n_act, :n] += F32(20)
        act = np.array([0, n_act - 1, 0, n_act - 1], np.uint8)
        ret, term = (rs.randn(batch) * 3).astype(F32), np.array([1, 0, 0, 0], np.uint8)
        isw = (rs.rand(batch) + 0.1).astype(F32)
        out = qr.qrdqn_loss(pred, tgt, None, act, ret, term, isw, n_act, n, dueling, GAMMA, 1.0)
        assert (out["a_next"] == 1 % n_act).all()
        p64 = torch.from_numpy(pred[:, :, :n].astype(np.float64)).requires_grad_()
        ref = ref_qr_loss(p64, torch.from_numpy(tgt[:, :, :n].astype(np.float64)), None, torch.from_numpy(act),
                          torch.from_numpy(ret), torch.from_numpy(term), torch.from_numpy(isw), GAMMA, 1.0, n_act, dueling)
        np.testing.assert_allclose(out["rows"], ref["rows"].numpy(), rtol=2e-4)
        np.testing.assert_allclose(out["dtheta"][:, :, :n], ref["grad"].numpy(), rtol=2e-4,
                                   atol=(n + 8) * 2.0 ** -24 * (1 + np.abs(out["T"]).max()) * isw.max())
        assert not out["dtheta"][:, :, n:].any()
        if dueling:                                             # the value row's gradient, and an action's share
            np.testing.assert_array_equal(out["dtheta"][:, n_act, :n], out["d"])
            assert out["dtheta"][:, n_act, :n].any()


# ---- FQF ---------------------------------------------------------------------------------------------------------------------

def _host_fractions(lg, n):
    """What the fractions kernel hands the loss kernel, with float64 exp / log rounded once: q, logq, then the fp32 chain."""
    f = fr.ref_fractions(torch.from_numpy(lg[:, :n].astype(np.float64)))
    q, logq = f["q"].numpy().astype(F32), f["logq"].numpy().astype(F32)
    tau, hat = qr.fqf_tau_chain(q)
    return dict(tau=tau, tau_hat=hat, q=q, logq=logq, H=qr.fqf_entropy(q, logq))


@pytest.mark.parametrize("n", [1, 2, 64])
def test_dominant_logits_repeat_the_fractions_at_both_ends_and_the_fraction_part_holds_its_bounds(n):
    rs = np.random.RandomState(n)
    batch, n_act, stride, n_stride, ent = qr.CORNER_BATCH, 3, 4, 68, 0.01
    lg = qr.dominant_logits(rs, batch, n, n_stride, rows=(0, qr.ROW_PLAIN))
    f = _host_fractions(lg, n)
    if n > 2:
        for b in (0, qr.ROW_PLAIN):
            assert (f["q"][b] == 0).sum() == n - 1 and f["q"][b, n // 2] == 1
            assert (f["tau"][b, :n // 2 + 1] == 0).all() and (f["tau"][b, n // 2 + 1:] == 1).all()
            assert set(f["tau_hat"][b].tolist()) == {0.0, 0.5, 1.0}      # tau_hat exactly 0 and exactly 1
            assert np.isfinite(f["logq"][b]).all()
    assert (f["tau"][:, 0] == 0).all() and (f["tau"][:, n] == 1).all() and (np.diff(f["tau"], axis=1) >= 0).all()
    # a zero weight contributes an exact 0 to the weighted Q
    theta = qr._blocks(rs, batch, n, n_act, stride, scale=1e6)
    wq = qr.wq_of_lane(theta, f["tau"], n_act)
    if n > 2:
        np.testing.assert_array_equal(wq[0], theta[0, n // 2, :n_act])
    # the whole loss against the float64 reference at the feature test's bounds
    c = qr.corner_case(n, n_act, n, n, stride, 1.0)
    mid = qr._blocks(rs, batch, max(n - 1, 1), n_act, stride)
    out = qr.fqf_loss(c["pred"], None if n == 1 else mid, f["tau"], f["tau_hat"], f["q"], f["logq"], f["H"], c["tgt"],
                      c["pol"], c["act"], c["ret"], c["term"], c["isw"], n_act, n_stride, GAMMA, 1.0, ent)
    assert not out["dlogits"][:, n:].any()
    t64 = lambda x: torch.from_numpy(np.asarray(x)[..., :n_act].astype(np.float64))    # noqa: E731
    f64 = {k: torch.from_numpy(v.astype(np.float64)) for k, v in f.items()}
    act = torch.from_numpy(qr.clamp_action(c["act"], n_act))
    ref = fr.ref_fqf_loss(t64(c["pred"]), None if n == 1 else t64(mid), f64, t64(c["tgt"]), t64(c["pol"]), act,
                          torch.from_numpy(c["ret"]), torch.from_numpy(c["term"]), torch.from_numpy(c["isw"]), GAMMA, 1.0, ent)
    atol, frac_atol = fr.dlogits_atol(ref, f64, n, ent)
    err = np.abs(out["dlogits"][:, :n].astype(np.float64) - ref["dlogits"].numpy())
    ratio = (err / np.maximum(atol.numpy(), 1e-300)).max()
    print("N %d: largest dlogits error / bound %.3f" % (n, ratio))
    assert (err <= atol.numpy()).all() and (np.abs(out["frac"] - ref["frac"].numpy()) <= frac_atol.numpy()).all()
    if n == 1:
        assert not out["dlogits"].any() and not out["frac"].any()
    if n == 2:
        assert (out["g"][:, 1] != 0).all() and not out["g"][:, 0].any()     # a single g_1


# ---- M-IQN -------------------------------------------------------------------------------------------------------------------

def test_one_action_and_a_dominant_action_make_the_soft_max_targets_exact():
    """A = 1: pi = 1 and lp = 0 exactly, T_j = returns_b + keep * (gamma_n * theta(j, 0)) -- arl_iqn_loss's targets; and a
    maximum unique by 88 tau_e: every other e_a is 0.  The emulation of munchausen_ref agrees bit for bit."""
    for tau_e in mr.TAUS_E:
        c = mr.miqn_case(5, 3, 5, 1, 4, 4, True)
        T = mr.emu_miqn_targets(c, mr.GAMMA, tau_e, alpha=mr.ALPHA)
        want = qr.stage_targets(c["ret"], c["term"], mr.GAMMA, c["nxt"], np.zeros(4, np.int64))
        np.testing.assert_array_equal(qr.bits(T), qr.bits(want))
