"""FQF on the device (csrc/fqf.hip: arl_fqf_fractions / _act / _loss; AtariFqfPolicy, FqfOptimizer, FQF).  The reference
has no FQF, so the yardsticks are the float64 restatements of tests/fqf_ref.py, which tests/test_fqf_host.py checks
against autograd through the integrated 1-Wasserstein distance.  Every bound is derived there (and in DESIGN.md, section
17) from the kernels' stated summation orders; every reference is built from the launch's own fp32 inputs cast up."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fqf_ref as R
from fqf_ref import EPS, POISON

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _f64(x):
    return torch.from_numpy(np.asarray(x, np.float64))


# ---- fractions ----------------------------------------------------------------------------------------------------

def _fractions(logits, n, only_serving=False):
    """logits fp32 [B][n_stride] (host) -> the kernel's outputs as host fp32 arrays (dict)."""
    from accel_rl_amd import _lib
    b = logits.shape[0]
    out = dict(tau=torch.full((b, n + 1), NAN, device=DEV), tau_hat=torch.full((b, n), NAN, device=DEV))
    if not only_serving:
        out.update(tau_mid=torch.full((b, max(n - 1, 1)), NAN, device=DEV) if n > 1 else None,
                   q=torch.full((b, n), NAN, device=DEV), logq=torch.full((b, n), NAN, device=DEV),
                   H=torch.full((b,), NAN, device=DEV))
        _lib.fqf_fractions(_dev(logits), n, out["tau"], out["tau_hat"].view(-1), None if n == 1 else out["tau_mid"].view(-1),
                           out["q"], out["logq"], out["H"])
    else:
        _lib.fqf_fractions(_dev(logits), n, out["tau"], out["tau_hat"].view(-1))
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _logits(rs, b, n, n_stride, lim=4.0):
    lg = np.full((b, n_stride), POISON, np.float32)
    lg[:, :n] = rs.uniform(-lim, lim, size=(b, n)).astype(np.float32)
    return lg


def _check_fractions(lg, n, got):
    b = lg.shape[0]
    ref = {k: v.numpy() for k, v in R.ref_fractions(_f64(lg[:, :n])).items()}
    q_rel, tau_atol, logq_atol, h_atol = R.fraction_bounds(lg[:, :n], n)
    tau, hat = got["tau"], got["tau_hat"]
    errs = dict(q=np.abs(got["q"] - ref["q"]).max(), tau=np.abs(tau - ref["tau"]).max(), tau_hat=np.abs(hat - ref["tau_hat"]).max(),
                logq=np.abs(got["logq"] - ref["logq"]).max(), H=np.abs(got["H"] - ref["H"]).max())
    print("B %d N %d: max err q %.3g  tau %.3g (bound %.3g)  tau_hat %.3g  logq %.3g (%.3g)  H %.3g (%.3g)" % (
        b, n, errs["q"], errs["tau"], tau_atol, errs["tau_hat"], errs["logq"], logq_atol, errs["H"], h_atol))
    for v in got.values():
        assert v is None or np.isfinite(v).all()
    assert (tau[:, 0] == 0.).all() and (tau[:, n] == 1.).all()              # exact properties
    assert (np.diff(tau, axis=1) >= 0).all()
    assert (hat >= tau[:, :-1]).all() and (hat <= tau[:, 1:]).all()
    if n > 1:
        np.testing.assert_array_equal(got["tau_mid"], tau[:, 1:n])          # the compact copy of the inner fractions
    # an underflowed q_k is an exact 0 where float64 still holds ~1e-87: 2^-126, the smallest normal number, covers it
    assert (np.abs(got["q"] - ref["q"]) <= q_rel * ref["q"] + 2.0 ** -126).all()
    assert errs["tau"] <= tau_atol and errs["tau_hat"] <= tau_atol
    assert errs["logq"] <= logq_atol and errs["H"] <= h_atol
    return ref


FRACTION_SHAPES = [(1, 1, 32), (3, 2, 32), (5, 8, 32), (2, 33, 64), (4, 64, 64), (257, 5, 32)]      # B, N, n_stride


@pytest.mark.parametrize("shape", FRACTION_SHAPES, ids=lambda s: "B%d-N%d-S%d" % s)
def test_fractions_vs_float64(shape):
    b, n, n_stride = shape
    lg = _logits(np.random.RandomState(7 * b + n), b, n, n_stride)
    got = _fractions(lg, n)
    _check_fractions(lg, n, got)
    if n == 1:
        assert (got["q"] == 1.).all() and (got["H"] == 0.).all() and (got["tau_hat"] == 0.5).all() and (got["logq"] == 0.).all()
    serving = _fractions(lg, n, only_serving=True)                          # the optional outputs left out: same fractions
    np.testing.assert_array_equal(serving["tau"], got["tau"])
    np.testing.assert_array_equal(serving["tau_hat"], got["tau_hat"])


def test_a_logit_far_below_the_rest_gives_an_exact_zero_and_a_finite_log():
    b, n, n_stride = 3, 8, 32
    lg = _logits(np.random.RandomState(1), b, n, n_stride)
    lg[0, 3] -= 200.
    lg[1, 0] -= 200.
    lg[2, n - 1] -= 200.
    got = _fractions(lg, n)
    _check_fractions(lg, n, got)
    for row, k in ((0, 3), (1, 0), (2, n - 1)):
        assert got["q"][row, k] == 0. and np.isfinite(got["logq"][row, k]) and got["logq"][row, k] < -190.
        assert got["tau"][row, k + 1] == got["tau"][row, k]                 # a zero-width interval


# ---- loss ---------------------------------------------------------------------------------------------------------

def _case(seed, n_act, n, stride, batch, double, weighted, uniform=False):
    """Inputs of one arl_fqf_loss launch (host fp32).  The fractions are the fractions kernel's own output for random
    logits (|l| <= 4; uniform: all-zero logits, dyadic fractions for N a power of two), so they are what the policy feeds
    the loss kernel; the selecting net is built by R.selecting under those weights."""
    rs = np.random.RandomState(seed)
    n_stride = (n + 3) // 4 * 4 + 4 * (seed % 2)
    lg = _logits(rs, batch, n, n_stride)
    if uniform:
        lg[:, :n] = 0.
    fr = _fractions(lg, n)
    w64 = np.diff(fr["tau"].astype(np.float64), axis=1)
    pred, tgt = R.block(rs, batch, n, n_act, stride), R.block(rs, batch, n, n_act, stride)
    mid = R.block(rs, batch, n - 1, n_act, stride) if n > 1 else None
    pol = R.block(rs, batch, n, n_act, stride) if double else None
    chosen = R.selecting(rs, pol if double else tgt, n_act, w64)
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    ret = (rs.randn(batch) * 3).astype(np.float32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    if batch > 1:
        term[0], term[1] = 1, 0                     # terminal and non-terminal rows in every case
    isw = (rs.rand(batch) + 0.1).astype(np.float32) if weighted else None
    return dict(pred=pred, mid=mid, tgt=tgt, pol=pol, act=act, ret=ret, term=term, isw=isw, chosen=chosen, fr=fr,
                n_stride=n_stride)


def _launch(c, n_act, gamma_n, kappa, ent_coef):
    from accel_rl_amd import _lib
    pred = _dev(c["pred"])
    batch, n, _ = pred.shape
    fr = c["fr"]
    dth = torch.full_like(pred, NAN)
    rows, pri, frac = (torch.full((batch,), NAN, device=DEV) for _ in range(3))
    dlg = torch.full((batch, c["n_stride"]), NAN, device=DEV)
    _lib.fqf_loss(pred, _dev(c["mid"]), _dev(fr["tau"]), _dev(fr["tau_hat"]), _dev(fr["q"]), _dev(fr["logq"]), _dev(fr["H"]),
                  _dev(c["tgt"]), _dev(c["pol"]), _dev(c["act"]), _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), n_act, n,
                  gamma_n, kappa, ent_coef, dth, rows, pri, dlg, frac)
    torch.cuda.synchronize()
    return dth.cpu(), rows.cpu(), pri.cpu(), dlg.cpu(), frac.cpu()


def _reference(c, n_act, gamma_n, kappa, ent_coef):
    cut = lambda x: None if x is None else _f64(x[:, :, :n_act])            # noqa: E731
    t = lambda x: None if x is None else torch.from_numpy(x)                # noqa: E731
    fr = {k: _f64(v) for k, v in c["fr"].items() if v is not None}
    pred = cut(c["pred"]).requires_grad_()
    ref = R.ref_fqf_loss(pred, cut(c["mid"]), fr, cut(c["tgt"]), cut(c["pol"]), t(c["act"]), t(c["ret"]), t(c["term"]),
                         t(c["isw"]), gamma_n, kappa, ent_coef)
    ar = torch.arange(pred.shape[0])
    if kappa > 0:                                   # autograd; the closed form must agree with it
        ref["grad"], = torch.autograd.grad(ref["rows"].sum(), pred)
        assert torch.allclose(ref["grad"][ar, :, t(c["act"]).long()], ref["dth"], rtol=1e-12, atol=1e-15)
    else:
        ref["grad"] = torch.zeros_like(pred)
        ref["grad"][ar, :, t(c["act"]).long()] = ref["dth"]
    ref["rows"] = ref["rows"].detach()
    ref["fr"] = fr
    th = pred.detach()[ar, :, t(c["act"]).long()]
    ref["min_u"] = (ref["T"][:, None, :] - th[:, :, None]).abs().min().item()
    ref["max_th"] = th.abs().max().item()
    return ref


def _check_against(ref, got, c, n_act, kappa, ent_coef):
    dth, rows, pri, dlg, frac = got
    batch, n, _ = dth.shape
    assert ref["margin"] >= 0.2 - 1e-6, ref["margin"]                       # every sample: no sample is skipped
    np.testing.assert_array_equal(ref["a_next"].numpy(), c["chosen"])
    w_max = ref["w"].max().item()
    t_max = ref["T"].abs().max().item()
    if kappa > 0:                                   # DESIGN.md section 15 with N' = N
        atol, rtol = (n + 8) * EPS * (1 + t_max / kappa) * w_max, 2e-4
    else:
        # plain quantile regression sees T only through [u < 0]: the case must keep every u away from the fp32 rounding of
        # T and of u itself (a property of the inputs, asserted), and then only the N-term chain rounds
        assert ref["min_u"] > 16 * EPS * (1 + t_max + ref["max_th"]), ref["min_u"]
        atol, rtol = (n + 8) * EPS * w_max, 0.
    err = (dth[:, :, :n_act].double() - ref["grad"]).abs()
    datol, fatol = R.dlogits_atol(ref, ref["fr"], n, ent_coef)
    derr = (dlg[:, :n].double() - ref["dlogits"]).abs()
    ferr = (frac.double() - ref["frac"]).abs()
    ratio = (derr / datol.clamp_min(1e-300)).max().item() if n > 1 else 0.
    print("margin %.3f  max|T| %.3f  grad atol %.3g  max grad err %.3g | max dlogits err %.3g of max |dlogits| %.3g, "
          "largest err / bound %.3g | frac_rows err / bound %.3g" % (
              ref["margin"], t_max, atol, err.max().item(), derr.max().item(), ref["dlogits"].abs().max().item(), ratio,
              (ferr / fatol.clamp_min(1e-300)).max().item() if n > 1 else 0.))
    for t in got:
        assert torch.isfinite(t).all()
    np.testing.assert_allclose(rows.double().numpy(), ref["rows"].numpy(), rtol=2e-4, atol=0)
    np.testing.assert_allclose(pri.double().numpy(), ref["loss_b"].clamp(1e-6, 1e6).numpy(), rtol=2e-4, atol=0)
    assert (err <= atol + rtol * ref["grad"].abs()).all(), err.max().item()
    other = torch.ones(dth.shape, dtype=torch.bool)                         # exact zeros outside the taken action's column
    other[torch.arange(batch), :, torch.from_numpy(c["act"]).long()] = False
    assert not dth[other].any()
    # the fraction loss: atol_bk = EPS w_b q_k [(2 N + 16) R_b + 8 ent_coef (|logq_k| + H_b)]  (tests/fqf_ref.py)
    assert (derr <= datol).all(), ratio
    assert (ferr <= fatol).all()
    assert not dlg[:, n:].any()                                             # exact zeros in the padding columns
    if n == 1:
        assert not dlg.any() and not frac.any()


LOSS_SHAPES = [(1, 1, 4, 1), (2, 2, 4, 3), (6, 8, 8, 32), (6, 33, 8, 2), (18, 64, 20, 5), (64, 5, 64, 2)]  # A, N, stride, B


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize("kappa", [1.0, 0.25, 0.0])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "A%d-N%d-S%d-B%d" % s)
def test_loss_gradients_and_fraction_gradient_vs_float64(shape, kappa, double, weighted, ent_coef):
    n_act, n, stride, batch = shape
    c = _case(100 * n_act + n + batch + 7 * int(double) + 3 * int(weighted), n_act, n, stride, batch, double, weighted)
    gamma_n = float(np.float32(0.99 ** 3))
    _check_against(_reference(c, n_act, gamma_n, kappa, ent_coef), _launch(c, n_act, gamma_n, kappa, ent_coef), c, n_act,
                   kappa, ent_coef)


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize("kappa", [1.0, 0.0])
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_quantile_part_equals_arl_iqn_loss_bit_for_bit(n, kappa, double):
    """All-zero logits and N a power of two: q = 1 / N, tau_i = i / N and tau_hat_i = (2 i + 1) / (2 N) are exact.  With
    tau_pred = tau_hat, N' = N and the same a* (both margins asserted) the two kernels run the same instructions."""
    from accel_rl_amd import _lib
    n_act, stride, batch = 6, 8, 5
    c = _case(40 + n, n_act, n, stride, batch, double, True, uniform=True)
    np.testing.assert_array_equal(c["fr"]["tau"], np.tile(np.arange(n + 1, dtype=np.float32) / n, (batch, 1)))
    np.testing.assert_array_equal(c["fr"]["tau_hat"], np.tile((2 * np.arange(n, dtype=np.float32) + 1) / (2 * n), (batch, 1)))
    ref = _reference(c, n_act, 0.97, kappa, 0.)
    sel = _f64((c["pol"] if double else c["tgt"])[:, :, :n_act])
    mean_q = sel.sum(dim=1) / n                                              # arl_iqn_loss's selection
    top2 = torch.topk(mean_q, 2, dim=1).values
    assert ref["margin"] >= 0.2 - 1e-6 and (top2[:, 0] - top2[:, 1]).min().item() >= 0.2 - 1e-6
    np.testing.assert_array_equal(mean_q.argmax(dim=1).numpy(), c["chosen"])
    np.testing.assert_array_equal(ref["a_next"].numpy(), c["chosen"])
    dth, rows, pri, _, _ = _launch(c, n_act, 0.97, kappa, 0.)
    pred = _dev(c["pred"])
    dth2 = torch.full_like(pred, NAN)
    rows2, pri2 = torch.full((batch,), NAN, device=DEV), torch.full((batch,), NAN, device=DEV)
    _lib.iqn_loss(pred, _dev(c["fr"]["tau_hat"]), _dev(c["tgt"]), _dev(c["pol"]), _dev(c["act"]), _dev(c["ret"]),
                  _dev(c["term"]), _dev(c["isw"]), n_act, n, n, 0.97, kappa, dth2, rows2, pri2)
    torch.cuda.synchronize()
    assert torch.isfinite(dth).all() and dth.any()
    assert torch.equal(dth, dth2.cpu()) and torch.equal(rows, rows2.cpu()) and torch.equal(pri, pri2.cpu())


# ---- action kernel ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_act,stride", [(1, 4), (6, 8), (64, 64)])
@pytest.mark.parametrize("k", [1, 33, 64])
def test_action_kernel_weighted_values_ties_zero_weights_override_and_onehot(k, n_act, stride):
    from accel_rl_amd import _lib
    b = 9                                           # two workgroups of four samples and one of one
    rs = np.random.RandomState(4 + k + n_act)
    tau = np.zeros((b, k + 1), np.float32)
    tau[:, 1:k] = np.sort(rs.uniform(0.02, 0.98, size=(b, k - 1)).astype(np.float32), axis=1)
    tau[:, k] = 1.
    zero_rows = []
    if k > 2:                                       # repeated fractions: zero weights at rows 4 and k - 2
        for j in (4, k - 2):
            tau[:, j + 1] = tau[:, j]
            zero_rows.append(j)
        tau[:, 1:k] = np.sort(tau[:, 1:k], axis=1)
        zero_rows = [j for j in range(k) if (tau[:, j + 1] == tau[:, j]).all()]
        assert len(zero_rows) >= 2
    w64 = np.diff(tau.astype(np.float64), axis=1)
    assert (w64 >= 0).all()
    theta = R.block(rs, b, k, n_act, stride)
    chosen = R.selecting(rs, theta, n_act, w64)
    for j in zero_rows:                             # what a zero weight multiplies must not count: large, finite, adversarial
        theta[:, j, :n_act] = np.float32(-1e30)
        theta[np.arange(b), j, (chosen + 1) % n_act] = np.float32(1e30)
    if n_act > 1:                                   # two bit-identical columns, both the maximum: the lower index wins
        lo, hi = 1, n_act - 1
        theta[5, :, hi] = theta[5, :, lo]
        theta[5, :, lo] += np.float32(2.0)
        theta[5, :, hi] += np.float32(2.0)
        for j in zero_rows:
            theta[5, j, hi] = theta[5, j, lo]
        chosen[5] = lo if lo != hi else chosen[5]
    q = R.ref_weighted_q(_f64(theta[:, :, :n_act]), _f64(tau))
    if n_act > 1:
        top2 = torch.topk(q, 2, dim=1).values
        assert ((top2[:, 0] - top2[:, 1])[torch.arange(b) != 5] >= 0.2 - 1e-6).all()
        if n_act > 2:
            q[5, n_act - 1] = -1e9                  # (float64 rounding must not pick between the twins)
    np.testing.assert_array_equal(q.argmax(dim=1).numpy(), chosen)
    ov = np.full(b, -1, np.int32)
    ov[::4] = rs.randint(0, n_act, size=len(ov[::4]))
    onehot = torch.full((b, n_act), NAN, device=DEV)
    greedy = torch.full((b,), 255, dtype=torch.uint8, device=DEV)
    _lib.fqf_act(_dev(theta), _dev(tau), _dev(ov), n_act, k, onehot, greedy)
    np.testing.assert_array_equal(greedy.cpu().numpy(), chosen)             # the argmax, override or not
    served = np.where(ov >= 0, ov, chosen)
    assert torch.equal(onehot.cpu(), F.one_hot(torch.from_numpy(served).long(), n_act).float())
    onehot2 = torch.full((b, n_act), NAN, device=DEV)
    _lib.fqf_act(_dev(theta), _dev(tau), None, n_act, k, onehot2, None)     # no override table, no greedy output
    assert torch.equal(onehot2.cpu(), F.one_hot(torch.from_numpy(chosen).long(), n_act).float())
    onehot3 = torch.full((b, n_act), NAN, device=DEV)                       # two launches: the same bits
    _lib.fqf_act(_dev(theta), _dev(tau), None, n_act, k, onehot3, None)
    assert torch.equal(onehot2, onehot3)


# ---- refusals -----------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    batch = 2
    big = torch.zeros(batch, 66, 68, device=DEV)                            # large enough for every size named below
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    vec = torch.zeros(batch * 70, device=DEV)
    nan = lambda *shape: torch.full(shape, NAN, device=DEV)                 # noqa: E731
    dth, rowsb, pri, frac, dlg, onehot = nan(batch, 66, 68), nan(batch), nan(batch), nan(batch), nan(batch, 72), nan(batch, 66)
    tau, hat, midt, qo, lqo, ho = nan(batch * 70), nan(batch * 70), nan(batch * 70), nan(batch * 70), nan(batch * 70), nan(batch)
    greedy = torch.full((batch,), 7, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                      # noqa: E731

    def fractions(lg=p(big), b=batch, n=8, s=8, t=p(tau), h=p(hat)):
        return lib.arl_fqf_fractions(lg, b, n, s, t, h, p(midt), p(qo), p(lqo), p(ho), None)

    def serve(th=p(big), t=p(vec), b=batch, a=6, n=8, s=8, out=p(onehot)):
        return lib.arl_fqf_act(th, t, None, b, a, n, s, out, p(greedy), None)

    def loss(pred=p(big), mid=p(big), b=batch, a=6, n=8, s=8, ns=8, kappa=1.0, ent=0.0, out=p(dth), dl=p(dlg), q=p(vec)):
        return lib.arl_fqf_loss(pred, mid, p(vec), p(vec), q, p(vec), p(vec), p(big), None, p(act), p(vec), p(act), None, b, a,
                                n, s, ns, 0.99, kappa, ent, out, p(rowsb), p(pri), dl, p(frac), None)

    for call in (fractions, serve, loss):
        assert call(n=0) == -1 and b"fractions" in lib.arl_last_error()
        assert call(n=65) == -1 and call(b=0) == -1
    for call in (serve, loss):
        assert call(a=65, s=68) == -1 and call(a=0) == -1                   # n_actions > 64, < 1
        assert call(s=10) == -1 and call(a=6, s=4) == -1                    # not a multiple of 4; a_stride < n_actions
    assert fractions(s=4) == -1 and fractions(s=10) == -1 and loss(ns=4) == -1 and loss(ns=10) == -1
    assert b"n_stride" in lib.arl_last_error()
    assert fractions(lg=None) == -1 and b"null" in lib.arl_last_error()
    assert fractions(t=None) == -1 and fractions(h=None) == -1
    assert serve(th=None) == -1 and serve(t=None) == -1 and serve(out=None) == -1
    assert loss(pred=None) == -1 and loss(mid=None) == -1 and loss(out=None) == -1 and loss(dl=None) == -1 and loss(q=None) == -1
    for bad in (-1.0, float("inf"), NAN):
        assert loss(kappa=bad) == -1 and b"kappa" in lib.arl_last_error()
        assert loss(ent=bad) == -1 and b"ent_coef" in lib.arl_last_error()
    assert fractions(lg=p(big) + 4) == -3 and loss(dl=p(dlg) + 4) == -3     # ARL_E_ALIGN
    torch.cuda.synchronize()
    for t in (dth, rowsb, pri, frac, dlg, onehot, tau, hat, midt, qo, lqo, ho):
        assert torch.isnan(t).all()
    assert (greedy == 7).all()
    assert fractions() == 0 and serve() == 0 and loss() == 0                # inside the limits they run
    assert loss(n=1, mid=None) == 0                                         # one fraction: no pass at inner fractions
    torch.cuda.synchronize()
    assert not torch.isnan(tau[:batch * 9]).any() and not torch.isnan(hat[:batch * 8]).any() and not torch.isnan(ho).any()
    assert not torch.isnan(onehot.view(-1)[:batch * 6]).any()
    assert not torch.isnan(dth.view(-1)[:batch * 8 * 8]).any() and not torch.isnan(dlg.view(-1)[:batch * 8]).any()


# ---- determinism --------------------------------------------------------------------------------------------------

def test_two_launches_of_each_kernel_are_bit_identical():
    n_act, n, stride, batch = 18, 51, 20, 37
    rs = np.random.RandomState(2)
    lg = _logits(rs, batch, n, 52)
    one, two = _fractions(lg, n), _fractions(lg, n)
    for k in one:
        np.testing.assert_array_equal(one[k], two[k])
    c = _case(11, n_act, n, stride, batch, True, True)
    for kappa in (1.0, 0.0):
        a, b = _launch(c, n_act, 0.97, kappa, 0.01), _launch(c, n_act, 0.97, kappa, 0.01)
        assert torch.isfinite(a[0]).all() and a[3].any()
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- policy, optimizer and algorithm ------------------------------------------------------------------------------------

N_ACT, BATCH, N_Q = 6, 8, 4


@pytest.fixture(scope="module")
def small():
    """AtariFqfPolicy on the small recipe of tests/test_iqn_gpu.py (2 conv layers, hidden 64, 6 actions, N = 4, batch 8):
    perturbed parameters, the fraction layer included so that q is not uniform, and a target net that differs."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(5)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = AtariFqfPolicy(epsilon=0.3, n_quantiles=N_Q, **spec)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT)), device=DEV)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    assert flat.size == policy.n_params == sum(int(np.prod(s)) for s in policy._ref_shapes)
    flat = flat + (rs.randn(flat.size) * 0.01).astype(np.float32)           # non-zero biases: layout errors would show
    policy.set_param_values(flat)
    np.testing.assert_array_equal(policy.get_param_values(), flat)          # round trip through the reference layout
    policy.flat_target.copy_(policy.flat_params * 0.9)
    b = BATCH
    mb = dict(obs=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
              nxt=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
              act=_dev(rs.randint(0, N_ACT, size=b).astype(np.uint8)), ret=_dev(rs.randn(b).astype(np.float32)),
              term=_dev((rs.rand(b) < 0.3).astype(np.uint8)), isw=_dev((rs.rand(b) + 0.2).astype(np.float32)))
    return policy, spec, mb


def _ref_psi(rp, spec, x):
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    return x.flatten(1), k


def _ref_theta(rp, k, psi, tau):
    """Plain float64 torch on the reference layout from the embedding on: tau [B][R] -> theta [B][R][A]."""
    c = torch.cos(np.pi * torch.arange(64, dtype=torch.float64) * tau[:, :, None])
    phi = F.relu(c @ rp[k] + rp[k + 1])
    h = F.relu((psi[:, None, :] * phi) @ rp[k + 2] + rp[k + 3])
    return h @ rp[k + 4] + rp[k + 5]


def _ref_params(policy, flat_bucket):
    fl = policy.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in policy._ref_shapes:
        m = int(np.prod(shape))
        out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    return out


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
def test_training_step_matches_autograd_through_plain_torch(small, double, ent_coef):
    """One FQF minibatch with the proposed fractions: gradients of every parameter in the reference's layout at the
    whole-step tolerances of tests/test_iqn_gpu.py; the fraction layer's slice against its own largest entry."""
    policy, spec, mb = small
    b, n = BATCH, N_Q
    assert policy.param_short_names == ["Conv0W", "Conv0b", "Conv1W", "Conv1b", "EmbW", "Embb", "FC0W", "FC0b", "OutputW",
                                        "Outputb", "FracW", "Fracb"]
    f = policy._f
    assert [tuple(s) for s in policy._ref_shapes[4:]] == [(64, f), (f,), (f, 64), (64,), (64, N_ACT), (N_ACT,), (f, n), (n,)]
    assert policy.frac_offset == policy._offsets[-2] and policy.frac_offset % 4 == 0
    gamma_n = float(np.float32(0.99))
    policy.flat_grads.fill_(NAN)
    rows, pri = policy.fqf_loss_and_grads(mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], gamma_n, 1.0,
                                          ent_coef, double_dqn=double)
    assert rows.data_ptr() + 4 * b == pri.data_ptr()            # the (2, b) buffer the optimizer's ring takes at once
    got = policy.bucket_to_reference(policy.flat_grads)
    kf = policy._k_frac
    assert not policy.grads[policy._k_head][N_ACT:].any() and not policy.grads[policy._k_head + 1][N_ACT:].any()
    assert not policy.grads[kf][n:].any() and not policy.grads[kf + 1][n:].any()    # exact zeros in both paddings
    assert torch.isfinite(policy.flat_grads).all()

    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    scale = float(np.float32(1. / 255))
    obs, nxt = mb["obs"].cpu().double() * scale, mb["nxt"].cpu().double() * scale
    psi, k = _ref_psi(rp, spec, obs)
    logits = psi.detach() @ rp[k + 6] + rp[k + 7]               # the fraction loss sends nothing into psi
    fr = R.ref_fractions(logits)
    frd = {key: v.detach() for key, v in fr.items()}
    pred = _ref_theta(rp, k, psi, frd["tau_hat"])
    with torch.no_grad():
        mid = _ref_theta(rp, k, psi, frd["tau"][:, 1:n])
        tgt = _ref_theta(rt, k, _ref_psi(rt, spec, nxt)[0], frd["tau_hat"])
        pol = _ref_theta(rp, k, _ref_psi(rp, spec, nxt)[0], frd["tau_hat"]) if double else None
    ref = R.ref_fqf_loss(pred, mid, frd, tgt, pol, mb["act"].cpu(), mb["ret"].cpu(), mb["term"].cpu(), mb["isw"].cpu(),
                         gamma_n, 1.0, ent_coef)
    assert ref["margin"] > 1e-4, ref["margin"]                  # the greedy next actions are away from fp32 ties
    loss = ref["rows"].sum()
    surrogate = (ref["w"] * ((ref["g"] * fr["tau"][:, 1:n]).sum(dim=1) - ent_coef * fr["H"])).sum()
    grads = torch.autograd.grad(loss + surrogate, rp)
    want = np.concatenate([g.detach().numpy().reshape(-1) for g in grads])
    n_frac = f * n + n
    main_got, main_want, frac_got, frac_want = got[:-n_frac], want[:-n_frac], got[-n_frac:], want[-n_frac:]
    q_host = frd["q"].numpy()
    print("loss %.6g vs %.6g; q in [%.3f, %.3f]; max grad err %.3g of max |grad| %.3g; fraction layer: %.3g of %.3g; "
          "entropy %.4f vs %.4f" % (rows.sum().item(), loss.item(), q_host.min(), q_host.max(),
                                    np.abs(main_got - main_want).max(), np.abs(main_want).max(),
                                    np.abs(frac_got - frac_want).max(), np.abs(frac_want).max(),
                                    policy.entropy.mean().item(), frd["H"].mean().item()))
    assert q_host.max() - q_host.min() > 1e-3                   # the perturbed fraction layer proposes non-uniform fractions
    assert abs(rows.sum().item() - loss.item()) <= 1e-4 * abs(loss.item())
    assert np.allclose(rows.cpu().numpy(), ref["rows"].detach().numpy(), rtol=2e-3, atol=1e-6)
    assert np.allclose(pri.cpu().numpy(), ref["loss_b"].clamp(1e-6, 1e6).numpy(), rtol=2e-3, atol=1e-5)
    assert np.allclose(main_got, main_want, rtol=2e-3, atol=2e-5 * max(np.abs(main_want).max(), 1e-3))
    assert np.abs(frac_want).max() > 0                          # the fraction layer learns
    assert np.allclose(frac_got, frac_want, rtol=2e-3, atol=2e-5 * np.abs(frac_want).max()), np.abs(frac_got - frac_want).max()
    assert np.allclose(policy.frac_rows.cpu().numpy(), ref["frac"].detach().numpy(), rtol=2e-3,
                       atol=2e-5 * ref["frac"].abs().max().item())
    assert np.allclose(policy.entropy.cpu().numpy(), frd["H"].numpy(), rtol=1e-4)


def _optimizer(policy, use_graph, lr=1e-4, frac_lr=1e-3, ent_coef=0.01):
    """FQF's optimizer and loss on `policy` (double DQN, importance weights), as FQF.initialize wires them."""
    from accel_rl_amd.algos.dqn.fqf import FQF
    algo = FQF(prioritized_replay=True, double_dqn=True, ent_coef=ent_coef,
               optimizer_args=dict(learning_rate=lr, use_graph=use_graph),
               fraction_optimizer_args=dict(learning_rate=frac_lr))
    inputs, loss = algo.build_loss(None, policy)
    algo.optimizer.initialize(inputs=inputs, loss=loss, target=policy)
    return algo.optimizer


def _inputs(mb):
    return (mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"])


@pytest.fixture()
def restored(small):
    """The module's policy with its parameters put back after the test."""
    policy, _, mb = small
    keep = policy.flat_params.clone()
    yield policy, mb
    policy.flat_params.copy_(keep)
    torch.cuda.synchronize()


def test_the_two_ranges_have_their_own_learning_rates(restored):
    from oracle import ref_port as P
    policy, mb = restored
    off = policy.frac_offset
    start = policy.flat_params.clone()
    _optimizer(policy, False, lr=1e-4, frac_lr=0.).optimize(_inputs(mb))
    after = policy.flat_params.clone()
    assert torch.equal(after[off:], start[off:]) and not torch.equal(after[:off], start[:off])
    assert (after[:off] != start[:off]).float().mean().item() > 0.1          # ... and the rest moved
    policy.flat_params.copy_(start)
    opt = _optimizer(policy, False, lr=0., frac_lr=1e-3)
    opt.optimize(_inputs(mb))
    after = policy.flat_params.clone()
    assert torch.equal(after[:off], start[:off]) and not torch.equal(after[off:], start[off:])
    # the fraction range took ONE RMSprop step (rho 0.95, epsilon 1e-5, from zero slots) on its own gradient, unclipped
    g = policy.flat_grads[off:].cpu().numpy()
    want, acc = P.rmsprop_step(start[off:].cpu().numpy(), g, np.zeros_like(g), 1e-3, rho=0.95, eps=1e-5)
    got = after[off:].cpu().numpy()
    assert np.abs(g).max() > 0 and np.allclose(got, want, rtol=1e-5, atol=1e-6), np.abs(got - want).max()
    assert np.allclose(opt._frac_slot0.cpu().numpy(), acc, rtol=1e-5, atol=1e-12)
    assert opt._frac_step_count.item() == 1. and opt._step_count.item() == 1.   # each range counts its own steps
    kf = policy._k_frac
    n = policy.n_quantiles
    assert not policy._w[kf].view(policy._n_stride, -1)[n:].any() and not policy._w[kf + 1][n:].any()   # the padding stays zero


def test_three_updates_eager_and_through_the_captured_graph_agree_bit_for_bit(restored):
    policy, mb = restored
    start = policy.flat_params.clone()
    eager = _optimizer(policy, False)
    for _ in range(3):
        eager.optimize(_inputs(mb))
    torch.cuda.synchronize()
    want = policy.flat_params.clone()
    assert torch.isfinite(want).all() and not torch.equal(want, start)
    policy.flat_params.copy_(start)
    graphed = _optimizer(policy, True)
    for _ in range(3):                              # two warm-up calls, then capture and replay (there is no RNG in this path)
        graphed.optimize(_inputs(mb))
    torch.cuda.synchronize()
    assert graphed._graph is not None
    assert torch.equal(policy.flat_params, want)
    assert torch.equal(graphed._frac_slot0, eager._frac_slot0) and torch.equal(graphed._slot0[:policy.frac_offset],
                                                                                 eager._slot0[:policy.frac_offset])
    assert torch.isfinite(policy.frac_rows).all() and torch.isfinite(policy.entropy).all()      # readable after the replay
    del graphed


def test_serving_split_does_not_change_the_actions(small):
    """11 rows at 3 rows a pass (three passes and a remainder of 2) against one pass: a row's fractions depend on that row
    alone, so the actions agree bit for bit."""
    policy, _, mb = small
    obs = torch.cat([mb["obs"], mb["nxt"]])[:11]
    policy.host_draws(1, 11, n_groups=1)
    policy.set_step(0)
    try:
        results = []
        for limit in (3 * policy.n_quantiles, 8192):
            policy.serve_pair_rows = limit
            greedy = policy.greedy_actions(obs).cpu()
            rows_last = policy.served_tau.shape[0]
            onehot = policy.prob_value(obs)[0].cpu()
            results.append((greedy, onehot, rows_last))
        assert results[0][2] == 2 and results[1][2] == 11
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
        assert (results[0][1].sum(dim=1) == 1).all()
        tau = policy.served_tau.cpu()
        assert (tau[:, 0] == 0).all() and (tau[:, -1] == 1).all() and (tau.diff(dim=1) >= 0).all()
    finally:
        policy.serve_pair_rows = 8192
        policy._overrides.clear()


def test_fqf_trains_with_prioritized_replay_and_eval():
    """The IQN end-to-end configuration at toy size with FQF: GpuVecEvalSampler -> device replay (prioritized) -> FQF
    updates (both ranges) inside the captured graph -> target sync, epsilon / beta schedules."""
    from accel_rl_amd.algos.dqn.fqf import FQF
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = FQF(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
               target_update_steps=64 * 3, reward_horizon=3, prioritized_replay=True, double_dqn=True, ent_coef=0.001,
               eps_greedy_args=dict(anneal_steps=64 * 10), fraction_optimizer_args=dict(learning_rate=1e-5))
    policy = AtariFqfPolicy(**cnn_specs[0], n_quantiles=8)
    first = {}
    initialize = policy.initialize

    def recording_initialize(*args, **kwargs):
        initialize(*args, **kwargs)
        first["params"] = policy.get_param_values()
    policy.initialize = recording_initialize
    runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9, eval_interval_steps=64 * 8)
    runner.train()
    tab = runner.last_tabular
    for key in ("StepsInEval", "TrajsInEval", "LossAverage", "PriorityAverage", "ReturnAverage", "ParamsNorm"):
        assert key in tab, key
    assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["TrajsInEval"] > 0
    assert 1e-6 <= tab["PriorityAverage"] <= 1e6
    assert algo._updates_per_optimize == 8 * 64 // 32 and abs(policy.get_epsilon() - 0.01) < 1e-9
    assert algo.replay_buffer.beta > 0.4
    final = policy.get_param_values()
    n_frac = policy._f * 8 + 8
    assert np.isfinite(final).all()
    assert not np.array_equal(final[:-n_frac], first["params"][:-n_frac])               # the network moved ...
    assert not np.array_equal(final[-n_frac:], first["params"][-n_frac:])               # ... and so did the fraction layer
    target = policy.bucket_to_reference(policy.flat_target)
    assert np.isfinite(target).all() and not np.array_equal(target, first["params"])    # the target net was synced
    assert torch.isfinite(policy.frac_rows).all() and torch.isfinite(policy.entropy).all()
    assert (policy.entropy > 0).all() and (policy.entropy <= np.log(8) + 1e-5).all()
    rs = np.random.RandomState(0)
    obs = _dev(rs.randint(0, 256, size=(5,) + tuple(policy._obs_shape), dtype=np.uint8))
    acts = policy.greedy_actions(obs).cpu().numpy()
    tau = policy.served_tau.cpu()
    assert (acts < policy.n_act).all() and tau.shape == (5, 9)
    assert (tau[:, 0] == 0).all() and (tau[:, -1] == 1).all() and (tau.diff(dim=1) >= 0).all()     # sorted, inside [0, 1]
