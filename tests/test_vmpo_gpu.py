"""V-MPO on the GPU: arl_vmpo_weights, arl_vmpo_head_loss_parts and arl_vmpo_dual_step (csrc/vmpo.hip) against the
float64 restatement tests/vmpo_ref.py, the policies' loss kind 4 against float64 autograd, and the learner -- captured
and replayed iterations equal to eager ones bit for bit, the duals moving, the weights handed to the head equal to the
restatement's selection.

The selection is compared exactly; psi and temp4 within one fp32 ulp of the float64 values rounded once
(r2d2_ref.within_one_ulp; for temp4[0..2] the ulp of the largest addend, whose terms may cancel).  The head kernel's
tolerance is the head tests' own (test_head_limits_gpu._tol: 2e-5 sqrt(k_red) max|want|), the whole-step one the project's
(rtol 2e-3, atol 2e-5 max |.|)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import autograd_ref
import ppg_ref
import resnet_ref as rr
import test_resnet_gpu as trg
import vmpo_ref
from r2d2_ref import within_one_ulp
from test_head_limits_gpu import _close, _head_inputs, _nan, _tol, _untouched
from test_ppg_gpu import _Float64Net, _assert_same_run, _aux_old, _cnn_setup, _weights, _whole_step_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _duals(eta, alpha):
    return torch.tensor([eta, alpha], dtype=torch.float32, device=DEV)


# ---- arl_vmpo_weights ------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 3, 64, 65, 1023, 1024, 1025, 4097, 65536]
EPS_ETA = 0.01


def _advantage_sets(n, rs):
    """[(name, advantages f32[n], eta, psi may underflow)]"""
    normal = rs.randn(n).astype(F32)
    dup = rs.randn(n).astype(F32)
    dup[rs.permutation(n)[:n // 2]] = np.sort(dup)[n // 2]      # half the rows hold the median: ties across the threshold
    zeros = rs.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=F32), size=n)
    zeros[rs.permutation(n)[:max(n - 2, 0)]] *= F32(0.)          # (mostly signed zeros)
    large = (rs.rand(n) * 200. - 100.).astype(F32)              # |A| / eta up to 1e4 at eta = 0.01
    return [("normal", normal, 0.7, False), ("equal", np.full(n, 1.25, dtype=F32), 1.0, False), ("dup", dup, 1.0, False),
            ("zeros", zeros, 0.5, False), ("large", large, 0.01, True), ("eta_floor", rs.randn(n).astype(F32), 1e-8, True)]


def _run_weights(L, full, idx, duals, n_rows):
    psi, temp4 = _nan(n_rows + 3), _nan(7)
    L.vmpo_weights(full, idx, duals, EPS_ETA, psi[:n_rows], temp4[:4])
    torch.cuda.synchronize()
    assert _untouched(psi[n_rows:]) and _untouched(temp4[4:])
    return psi[:n_rows].cpu().numpy(), temp4[:4].cpu().numpy()


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("n", SIZES)
def test_weights_vs_float64(L, n, with_idx):
    rs = np.random.RandomState(3 * n + with_idx)
    for name, adv, eta, underflow in _advantage_sets(n, rs):
        n_rows = 2 * n if with_idx else n
        rows = rs.permutation(n_rows)[:n].astype(np.int32) if with_idx else np.arange(n, dtype=np.int32)
        full = rs.randn(n_rows).astype(F32) * F32(50.)              # (rows outside the minibatch: never read)
        full[rows] = adv
        idx = torch.from_numpy(rows).to(DEV) if with_idx else None
        duals = _duals(eta, 5.0)
        full_d = torch.from_numpy(full).to(DEV)
        psi, temp4 = _run_weights(L, full_d, idx, duals, n_rows)
        ref = vmpo_ref.weights(adv, eta, EPS_ETA)
        want = ref["psi"].astype(F32)
        got = psi[rows]
        outside = np.ones(n_rows, dtype=bool)
        outside[rows] = False
        assert np.isnan(psi[outside]).all(), name                    # rows outside the minibatch keep their fill
        assert (got[~ref["sel"]] == 0).all(), name                   # unselected rows are exactly 0
        if not underflow:
            assert np.array_equal(got > 0, ref["sel"]), name         # the selected set is the reference's
        else:
            assert (got[want > 0] > 0).all(), name
        assert within_one_ulp(got, want).all(), (name, np.abs(got - want).max())
        assert temp4[3] == ref["n_top"] == (n + 1) // 2
        for k, key in enumerate(("temp_loss", "d_eta", "L")):
            ulp = np.spacing(F32(max(ref["addends"][k], abs(ref[key]))))
            print("n %6d %-9s %-9s want % .9g got % .9g ulp %.3g" % (n, name, key, ref[key], temp4[k], ulp))
            assert np.isfinite(temp4[k]) and abs(float(temp4[k]) - ref[key]) <= ulp, (name, key)
        psi2, temp4_2 = _run_weights(L, full_d, idx, duals, n_rows)  # two launches give the same bits
        assert np.array_equal(psi.view(np.uint32), psi2.view(np.uint32)), name
        assert np.array_equal(temp4.view(np.uint32), temp4_2.view(np.uint32)), name


def test_weights_refusals_leave_the_fill(L):
    lib = L.load()
    adv = torch.randn(8, device=DEV)
    duals = _duals(1.0, 5.0)
    psi, temp4 = _nan(8), _nan(4)
    for n in (0, 65537):
        assert lib.arl_vmpo_weights(adv.data_ptr(), None, n, duals.data_ptr(), 0.01, psi.data_ptr(), temp4.data_ptr(),
                                    L.stream_ptr()) == -2
    for args in ((None, duals.data_ptr(), psi.data_ptr(), temp4.data_ptr()),
                 (adv.data_ptr(), None, psi.data_ptr(), temp4.data_ptr()),
                 (adv.data_ptr(), duals.data_ptr(), None, temp4.data_ptr()),
                 (adv.data_ptr(), duals.data_ptr(), psi.data_ptr(), None)):
        assert lib.arl_vmpo_weights(args[0], None, 8, args[1], 0.01, args[2], args[3], L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert _untouched(psi) and _untouched(temp4)


# ---- arl_vmpo_head_loss_parts ----------------------------------------------------------------------------------------------

HEAD_CASES = [(1, 1, 1), (2, 4, 3), (17, 60, 15), (6, 64, 5), (18, 128, 1025), (6, 512, 4097), (18, 1024, 1),
              (18, 1024, 4097)]
VARIANTS = [(i, m, c) for i in (True, False) for m in (True, False) for c in (True, False)]     # idx, relu mask, inv_count
_case_id = lambda c: "A%d-hid%d-B%d" % c                                                       # noqa: E731
_var_id = lambda v: "%s-%s-%s" % (("idx" if v[0] else "rows"), ("mask" if v[1] else "nomask"),  # noqa: E731
                                  ("inv" if v[2] else "mean"))
ETA, ALPHA, C_V = 0.7, 3.5, 0.5


def _launch(L, h, w, b, act, psi, ret, old, idx, duals, inv, c_v, mask_dh):
    """One arl_vmpo_head_loss_parts + the fold, every output inside a larger NaN-filled buffer."""
    batch, hid = h.shape
    K = w.shape[0]
    o = dict(dout=_nan(batch + 1, K), dh=_nan(batch + 1, hid), dw=_nan(K + 1, hid), db=_nan(K + 4), loss4=_nan(5))
    folds = L.FoldList()
    folds.vmpo_head_loss(h, w, b, act, psi, ret, old, idx, duals, inv, K - 1, c_v, o["dout"][:batch], o["dh"][:batch],
                         o["dw"][:K], o["db"][:K], o["loss4"][:4], L.pg_head_workspace(DEV), relu_mask_dh=mask_dh)
    folds.run()
    torch.cuda.synchronize()
    assert _untouched(o["dout"][batch]) and _untouched(o["dh"][batch]) and _untouched(o["dw"][K])
    assert _untouched(o["db"][K:]) and _untouched(o["loss4"][4:])
    return dict(dout=o["dout"][:batch], dh=o["dh"][:batch], dw=o["dw"][:K], db=o["db"][:K], loss4=o["loss4"][:4])


def _head_setup(case, with_idx, salt=0):
    """_head_inputs, stored probabilities with exact zeros, and psi of the minibatch's advantages from the restatement
    (fp32, NaN on every row outside the minibatch: the kernel reads psi by idx alone)."""
    n_act, hid, batch = case
    gen, h, w, b, act, adv, ret, idx = _head_inputs(n_act, hid, batch, 13 * hid + n_act + batch + 5 + salt)
    if not with_idx:
        idx = None
    sel = torch.arange(batch, device=DEV) if idx is None else idx.long()
    old = _aux_old(gen, ret.numel(), n_act)
    psi = _nan(ret.numel())
    ref = vmpo_ref.weights(adv[sel].cpu().numpy(), ETA, EPS_ETA)
    psi[sel] = torch.from_numpy(ref["psi"].astype(F32)).to(DEV)
    return dict(h=h, w=w, b=b, act=act, ret=ret, idx=idx, sel=sel, old=old, psi=psi, gen=gen)


@pytest.mark.parametrize("variant", VARIANTS, ids=_var_id)
@pytest.mark.parametrize("case", HEAD_CASES, ids=_case_id)
def test_head_vs_float64(L, case, variant):
    n_act, hid, batch = case
    with_idx, mask_dh, with_inv = variant
    s = _head_setup(case, with_idx)
    inv, wgt = _weights(batch, with_inv)
    got = _launch(L, s["h"], s["w"], s["b"], s["act"], s["psi"], s["ret"], s["old"], s["idx"], _duals(ETA, ALPHA), inv,
                  C_V, mask_dh)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k                      # (stored probabilities with exact zeros)
    h64, w64, b64 = s["h"].double(), s["w"].double(), s["b"].double()
    prob, value, _ = ppg_ref.head(h64, w64, b64, n_act)
    sel = s["sel"]
    a, psi, ret, old = s["act"][sel].long(), s["psi"][sel].double(), s["ret"][sel].double(), s["old"][sel].double()
    alpha = float(F32(ALPHA))
    dout = vmpo_ref.dout(prob, value, a, psi, ret, old, alpha, C_V, wgt)
    dh, dw, db = ppg_ref.head_grads(dout, h64, w64, n_act, stop_value=False)
    if mask_dh:
        dh = dh * (s["h"] > 0)
    K = n_act + 1
    _close(got["dout"], dout, K, "dout")
    _close(got["dh"], dh, K, "dh")
    _close(got["dw"], dw, batch, "dw")
    _close(got["db"], db, batch, "db")
    pa = prob[torch.arange(batch, device=DEV), a]
    rows3 = [-psi * torch.log(pa + 1e-8), C_V * wgt * (value - ret) ** 2,
             wgt[:, None] * old * (torch.log(old + 1e-8) - torch.log(prob + 1e-8))]
    want = [r.sum().item() for r in rows3]
    scale = [r.abs().sum().item() for r in rows3]
    want.append(sum(want))                                           # [3]: the plain sum, the KL not scaled by alpha
    scale.append(sum(scale))
    for i in range(4):
        err = abs(got["loss4"][i].item() - want[i])
        assert err <= 1e-5 * (scale[i] + 1.), (i, err, scale[i])


@pytest.mark.parametrize("case", HEAD_CASES, ids=_case_id)
def test_head_at_zero_weights_at_its_own_probabilities_and_next_to_the_auxiliary_phase(L, case):
    n_act, hid, batch = case
    s = _head_setup(case, True, salt=2)
    zero_psi = torch.zeros_like(s["psi"])
    args = (s["h"], s["w"], s["b"], s["act"])
    # psi all zero and alpha = 0: nothing reaches the logits
    got = _launch(L, *args, zero_psi, s["ret"], s["old"], s["idx"], _duals(ETA, 0.0), None, C_V, True)
    assert not got["dout"][:, :n_act].any() and got["loss4"][0].item() == 0.
    assert bool((got["dout"][:, n_act] != 0).any())
    # the value column is arl_ppg_head_loss_parts' auxiliary phase's, bit for bit
    full = _launch(L, *args, s["psi"], s["ret"], s["old"], s["idx"], _duals(ETA, ALPHA), None, C_V, True)
    K = n_act + 1
    aux = dict(dout=_nan(batch, K), dh=_nan(batch, hid), dw=_nan(K, hid), db=_nan(K), loss4=_nan(4))
    folds = L.FoldList()
    folds.ppg_head_loss(s["h"], s["w"], s["b"], None, None, s["ret"], s["old"], s["idx"], None, None, n_act, L.PPG_AUX,
                        0., C_V, 0., 1.0, aux["dout"], aux["dh"], aux["dw"], aux["db"], aux["loss4"],
                        L.pg_head_workspace(DEV), relu_mask_dh=True)
    folds.run()
    torch.cuda.synchronize()
    assert torch.equal(full["dout"][:, n_act], aux["dout"][:, n_act]) and torch.equal(got["dout"][:, n_act],
                                                                                        aux["dout"][:, n_act])
    assert full["loss4"][1].item() == aux["loss4"][1].item()
    # old_prob = the kernel's own probabilities, psi = 0: the KL and its gradient vanish within the tolerance
    own, v_k = torch.empty(batch, n_act, device=DEV), torch.empty(batch, device=DEV)
    L.pg_head_infer(s["h"], s["w"], s["b"], own, v_k)
    rows = s["ret"][:batch].contiguous()
    got = _launch(L, *args[:3], s["act"][:batch].contiguous(), zero_psi[:batch].contiguous(), rows, own, None,
                  _duals(ETA, ALPHA), None, C_V, False)
    zeros = torch.zeros(batch, n_act, dtype=torch.float64, device=DEV)
    _close(got["dout"][:, :n_act], zeros, n_act + 1, "dout at old == p", scale=ALPHA / batch)
    assert abs(got["loss4"][2].item()) <= _tol(zeros, n_act + 1, scale=1.)


def test_head_two_launches_give_the_same_bits(L):
    for case in ((6, 512, 4097), (18, 128, 1025), (17, 60, 15)):
        s = _head_setup(case, True, salt=9)
        run = lambda: _launch(L, s["h"], s["w"], s["b"], s["act"], s["psi"], s["ret"], s["old"], s["idx"],   # noqa: E731
                              _duals(ETA, ALPHA), None, C_V, True)
        first, second = run(), run()
        for k in first:
            assert torch.equal(first[k], second[k]), (case, k)


def test_head_refusals_launch_nothing_and_the_limits_run(L):
    batch = 8
    lib = L.load()
    h = torch.rand(batch, 1025, device=DEV)
    w, b = torch.rand(20, 1025, device=DEV), torch.rand(20, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    psi, ret = torch.rand(batch, device=DEV), torch.rand(batch, device=DEV)
    old, duals = torch.rand(batch, 19, device=DEV), _duals(1.0, 5.0)
    ws = L.pg_head_workspace(DEV)
    o = dict(dout=_nan(batch, 20), dh=_nan(batch, 1025), dw=_nan(20, 1025), db=_nan(20), loss4=_nan(4))
    items = (L.ArlFoldItem * 3)()
    base = dict(h=h.data_ptr(), w=w.data_ptr(), b=b.data_ptr(), act=act.data_ptr(), psi=psi.data_ptr(),
                ret=ret.data_ptr(), old=old.data_ptr(), idx=None, duals=duals.data_ptr(), inv=None, n=batch, hid=64,
                n_act=4, c_v=0.5, mask=0, dout=o["dout"].data_ptr(), dh=o["dh"].data_ptr(), dw=o["dw"].data_ptr(),
                db=o["db"].data_ptr(), loss4=o["loss4"].data_ptr(), ws=ws.data_ptr(),
                items=ctypes.cast(items, ctypes.c_void_p))

    def call(**kw):
        a = dict(base, **kw)
        return lib.arl_vmpo_head_loss_parts(
            a["h"], a["w"], a["b"], a["act"], a["psi"], a["ret"], a["old"], a["idx"], a["duals"], a["inv"], a["n"],
            a["hid"], a["n_act"], a["c_v"], a["mask"], a["dout"], a["dh"], a["dw"], a["db"], a["loss4"], a["ws"],
            a["items"], L.stream_ptr())

    for kw in (dict(n_act=0), dict(n_act=19), dict(hid=0), dict(hid=1025), dict(n=0), dict(n=1 << 31)):
        assert call(**kw) == -2, kw
    for name in ("h", "w", "b", "act", "psi", "ret", "old", "duals", "dout", "dh", "dw", "db", "loss4", "ws", "items"):
        assert call(**{name: None}) == -1 and b"null" in lib.arl_last_error(), name
    for bad in (NAN, float("inf"), -float("inf")):
        assert call(c_v=bad) == -1 and b"v_loss_coeff" in lib.arl_last_error()
    torch.cuda.synchronize()
    for name, t in o.items():
        assert _untouched(t), name
    assert all(it.part is None and it.out is None for it in items)
    # the limits themselves run: 18 actions x 1024 hidden units
    assert call(n_act=18, hid=1024) == 0
    L._check(lib.arl_fold_many(items, 3, L.stream_ptr()), "arl_fold_many")
    torch.cuda.synchronize()
    assert torch.isfinite(o["dout"].view(-1)[:batch * 19]).all() and torch.isfinite(o["loss4"]).all()


# ---- arl_vmpo_dual_step ----------------------------------------------------------------------------------------------------

class _OptRig(object):
    """arl_opt_step on a two-element bucket: the reference the dual step must equal bit for bit."""

    def __init__(self, L, adam, init):
        z = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)                             # noqa: E731
        self.p, self.g, self.s0, self.s1 = z(4), z(4), z(4), (z(4) if adam else None)
        self.p[:2] = torch.tensor(init, device=DEV)
        self.t, self.lr_mult = z(1), torch.full((1,), 0.6, device=DEV)
        self.partials = torch.zeros(L.OPT_PARTIALS, dtype=torch.float64, device=DEV)
        st = L.ArlOptState()
        st.n_params = 2
        st.params, st.grads, st.slot0 = self.p.data_ptr(), self.g.data_ptr(), self.s0.data_ptr()
        st.slot1 = self.s1.data_ptr() if adam else None
        st.step_count, st.lr_mult, st.partials = self.t.data_ptr(), self.lr_mult.data_ptr(), self.partials.data_ptr()
        st.grad_norm_log, st.norm_log_len = None, 0
        self.st = st


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_dual_step_equals_the_flat_bucket_update_then_the_projection(L, method):
    adam = method == "adam"
    kid = L.OPT_ADAM if adam else L.OPT_RMSPROP
    lr, (b1, b2, eps) = 3e-2, ((0.9, 0.999, 1e-8) if adam else (0.9, 0.0, 1e-6))
    eps_alpha = 0.005
    init = (1.0, 5.0)
    rig = _OptRig(L, adam, init)
    duals = _nan(5)
    duals[:2] = torch.tensor(init, device=DEV)
    s0, s1, t = torch.zeros(2, device=DEV), (torch.zeros(2, device=DEV) if adam else None), torch.zeros(1, device=DEV)
    temp4, loss4 = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    for step, (d_eta, kl) in enumerate([(0.37, 0.02), (-1.9, 0.0007), (0.004, 0.3)]):
        temp4.copy_(torch.tensor([NAN, d_eta, NAN, NAN]))           # (only [1] is read)
        loss4.copy_(torch.tensor([NAN, NAN, kl, NAN]))              # (only [2] is read)
        L.vmpo_dual_step(duals[:2], s0, s1, t, rig.lr_mult, temp4, loss4, eps_alpha, kid, lr, b1, b2, eps)
        rig.g[:2] = torch.stack([temp4[1], torch.tensor(eps_alpha, dtype=torch.float32, device=DEV) - loss4[2]])
        L.opt_step(rig.st, kid, lr, 1.0, None, b1, b2, eps)
        rig.p.clamp_(min=1e-8)
        torch.cuda.synchronize()
        assert torch.equal(duals[:2], rig.p[:2]) and _untouched(duals[2:]), (step, duals, rig.p)
        assert torch.equal(s0, rig.s0[:2]) and (not adam or torch.equal(s1, rig.s1[:2]))
        assert t.item() == rig.t.item() == step + 1
    assert bool((duals[:2] != torch.tensor(init, device=DEV)).all()) and bool((duals[:2] >= 1e-8).all())


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_dual_step_that_would_go_negative_lands_on_the_floor(L, method):
    adam = method == "adam"
    kid = L.OPT_ADAM if adam else L.OPT_RMSPROP
    b1, b2, eps = (0.9, 0.999, 1e-8) if adam else (0.9, 0.0, 1e-6)
    duals = _duals(1e-3, 2e-3)
    s0, s1, t = torch.zeros(2, device=DEV), (torch.zeros(2, device=DEV) if adam else None), torch.zeros(1, device=DEV)
    temp4 = torch.tensor([0., 4.0, 0., 0.], device=DEV)             # eta's gradient > 0: eta goes down by ~lr
    loss4 = torch.tensor([0., 0., 0.0, 0.], device=DEV)             # KL 0 < eps_alpha: alpha goes down too
    L.vmpo_dual_step(duals, s0, s1, t, torch.ones(1, device=DEV), temp4, loss4, 0.005, kid, 0.5, b1, b2, eps)
    torch.cuda.synchronize()
    assert duals.cpu().numpy().tolist() == [float(F32(1e-8))] * 2 and t.item() == 1.


# ---- policies --------------------------------------------------------------------------------------------------------------

def _psi_for(adv, rows, n_rows):
    """fp32 psi over `rows` of an [n_rows] batch from the restatement; NaN elsewhere."""
    ref = vmpo_ref.weights(adv[rows], ETA, EPS_ETA)
    psi = np.full(n_rows, np.nan, dtype=F32)
    psi[rows] = ref["psi"].astype(F32)
    return psi


@pytest.mark.parametrize("gather", [True, False], ids=["idx", "rows"])
def test_cnn_policy_kind_4_matches_float64_autograd(gather):
    policy, data, idx = _cnn_setup()
    idx = idx if gather else None
    sel = torch.arange(40) if idx is None else idx.cpu().long()
    n = sel.numel()
    psi32 = _psi_for(data["advantages"].cpu().numpy(), sel.numpy(), 40)
    mb = dict(data, idx=idx, psi=torch.from_numpy(psi32).to(DEV))
    duals = _duals(ETA, ALPHA)
    policy.flat_grads.fill_(NAN)
    loss4 = policy.loss_and_grads(mb, 4, 0., C_V, 0., torch.ones(1, device=DEV), duals=duals).cpu().numpy()
    got = [g.detach().cpu().numpy().copy() for g in policy.grads]
    net = _Float64Net(policy)
    x = policy._scaled_f32(data["observations"], idx)[:, :policy._c_in].cpu().double()
    pick = lambda k: data[k].cpu()[sel]                                                      # noqa: E731
    wgt = torch.full((n,), 1. / n, dtype=torch.float64)
    prob, value = autograd_ref.forward(net, x)
    pi, v, akl, kl = vmpo_ref.losses(prob, value, pick("actions").long(), torch.from_numpy(psi32[sel.numpy()]).double(),
                                     pick("returns").double(), pick("old_prob").double(), float(F32(ALPHA)), C_V, wgt)
    want = [g.numpy() for g in torch.autograd.grad(pi + v + akl, net.params)]
    terms = np.array([float(t.detach()) for t in (pi, v, kl)])
    _whole_step_close(loss4[:3], terms, np.abs(terms).max(), "losses")
    assert abs(loss4[3] - terms.sum()) <= 2e-3 * np.abs(terms).sum()
    scale = max(max(np.abs(g).max() for g in want), 1e-3)
    assert all(np.isfinite(g).all() for g in got)
    for k, (g, wv) in enumerate(zip(got, want)):
        assert np.abs(wv).max() > 0, k
        _whole_step_close(g, wv, scale, "kind 4 param %d" % k)
    with pytest.raises(NotImplementedError, match="valids"):
        policy.loss_and_grads(dict(mb, valids=torch.ones(40, dtype=torch.int8, device=DEV)), 4, 0., C_V, 0.,
                              torch.ones(1, device=DEV), duals=duals)
    with pytest.raises(TypeError, match="duals"):
        policy.loss_and_grads(mb, 4, 0., C_V, 0., torch.ones(1, device=DEV))


def test_cnn_policy_kind_4_walked_in_passes_gives_the_one_pass_gradient():
    """24 rows in passes of 8: psi was normalised over the whole minibatch before the passes, the KL and the value loss
    are normalised by the whole minibatch's count."""
    policy, data, idx = _cnn_setup()
    psi32 = _psi_for(data["advantages"].cpu().numpy(), idx.cpu().numpy().astype(np.int64), 40)
    mb = dict(data, idx=idx, psi=torch.from_numpy(psi32).to(DEV))
    duals, lr_mult = _duals(ETA, ALPHA), torch.ones(1, device=DEV)
    try:
        policy.max_rows_per_pass = None
        loss_one = policy.loss_and_grads(mb, 4, 0., C_V, 0., lr_mult, duals=duals).clone()
        one = [g.clone() for g in policy.grads]
        policy.max_rows_per_pass = 8
        loss_p = policy.loss_and_grads(mb, 4, 0., C_V, 0., lr_mult, duals=duals).clone()
        passes = [g.clone() for g in policy.grads]
    finally:
        policy.max_rows_per_pass = None
    assert torch.allclose(loss_p, loss_one, rtol=2e-3, atol=2e-5 * loss_one.abs().max().item()), (loss_p, loss_one)
    scale = max(max(g.abs().max().item() for g in one), 1e-3)
    for g1, gp in zip(one, passes):
        assert torch.allclose(gp, g1, rtol=2e-3, atol=2e-5 * scale), (gp - g1).abs().max().item()


@functools.lru_cache(maxsize=None)
def _resnet_reference(name, gather):
    """The float64 step of test_resnet_gpu.reference_step for kind 4: same parameters, observations, targets and
    behaviour probabilities."""
    cfg, arr = trg.CASES[name], trg.case_arrays(name)
    ppo = trg.reference_step(name, 1, gather)
    rp, pos = [], 0
    for _, shape in trg._layout(name):
        m = int(np.prod(shape))
        rp.append(torch.from_numpy(arr["flat"][pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    rows = arr["idx"].astype(np.int64) if gather else np.arange(cfg["batch"])
    x = torch.from_numpy(arr["obs"][rows].astype(np.float64)) * np.float64(F32(1. / 255))
    prob, value, taps = rr.ref_net(rp, cfg["channels"], cfg["blocks"], len(cfg["hidden"]), cfg["n_act"], x)
    pick = lambda a: torch.from_numpy(a[rows].astype(np.float64))                              # noqa: E731
    n = len(rows)
    psi32 = _psi_for(arr["advantages"].astype(F32), rows, len(arr["advantages"]))
    wgt = torch.full((n,), 1. / n, dtype=torch.float64)
    act = torch.from_numpy(arr["actions"][rows].astype(np.int64))
    pi, v, akl, kl = vmpo_ref.losses(prob, value, act, torch.from_numpy(psi32[rows]).double(), pick(arr["returns"]),
                                     pick(ppo["old_prob"]), float(F32(ALPHA)), trg.V_COEFF, wgt)
    grads = list(torch.autograd.grad(pi + v + akl, rp))
    return dict(losses=np.array([float(t.detach()) for t in (pi, v, kl)]), grads=[g.numpy() for g in grads],
                margin=rr.branch_margin(taps), old_prob=ppo["old_prob"], names=[n_ for n_, _ in trg._layout(name)],
                psi=psi32)


@pytest.mark.parametrize("gather", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("name", sorted(trg.CASES))
def test_resnet_policy_kind_4_matches_float64_autograd(name, gather):
    cfg, arr = trg.CASES[name], trg.case_arrays(name)
    ref = _resnet_reference(name, gather)
    assert ref["margin"] > rr.BRANCH_MARGIN, ref["margin"]
    policy = trg._make_policy(name)
    policy.set_param_values(arr["flat"])
    batch = cfg["batch"]
    cut = (lambda a: a) if gather else (lambda a: a[:batch])
    dev = trg._dev
    mb = dict(observations=dev(cut(arr["obs"])), idx=dev(arr["idx"]) if gather else None,
              actions=dev(cut(arr["actions"])), returns=dev(cut(arr["returns"])), old_prob=dev(cut(ref["old_prob"])),
              psi=dev(cut(ref["psi"])))
    policy.flat_grads.fill_(NAN)
    loss4 = trg._host(policy.loss_and_grads(mb, 4, 0., trg.V_COEFF, 0., torch.ones(1, device=DEV),
                                            duals=_duals(ETA, ALPHA)))
    got_flat = policy.bucket_to_reference(policy.flat_grads)
    _whole_step_close(loss4[:3], ref["losses"], np.abs(ref["losses"]).max(), "losses")
    assert abs(float(loss4[3]) - ref["losses"].sum()) <= 2e-3 * np.abs(ref["losses"]).sum()
    want_flat = np.concatenate([g.reshape(-1) for g in ref["grads"]])
    assert np.isfinite(got_flat).all() and got_flat.size == want_flat.size
    scale, pos = max(np.abs(want_flat).max(), 1e-3), 0
    for gname, want in zip(ref["names"], ref["grads"]):
        got = got_flat[pos:pos + want.size].reshape(want.shape)
        pos += want.size
        assert np.abs(want).max() > 0, gname
        _whole_step_close(got, want, scale, "%s kind 4 %s" % (name, gname))


# ---- learner ---------------------------------------------------------------------------------------------------------------

def _train(use_graph, n_itr, resnet=False, wrap=None):
    """V-MPO on the synthetic pong, 8 envs x horizon 5: two epochs of two minibatches of 20 rows.  wrap(algo, policy):
    called once initialize has run."""
    from accel_rl_amd.algos.pg import VMPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=2, envs_per=2,
                            max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = VMPO(optimizer_args=dict(epochs=2, minibatch_size=20, learning_rate=1e-3), use_graph=use_graph)
    policy = AtariResnetPolicy() if resnet else AtariCnnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    log = dict(infos=[])
    initialize, optimize = algo.initialize, algo.optimize_policy

    def watching_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()
        if wrap is not None:
            wrap(algo, policy)

    def recording_optimize(itr, samples):
        out = optimize(itr, samples)
        log["infos"].append(out[1])
        return out
    algo.initialize, algo.optimize_policy = watching_initialize, recording_optimize
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=40 * (n_itr - 1), seed=9, log_interval_steps=40)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: trg._host(v).copy() for k, v in info.items()} for info in log["infos"]]
    log["duals"] = trg._host(algo.optimizer.duals).copy()
    return algo, policy, log


def _assert_trained(algo, policy, log, n_itr):
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"]) and len(log["infos"]) == n_itr
    assert algo.optimizer._n_minibatches == 4 and algo.optimizer._dual_step_count.item() == 4 * n_itr
    for info in log["infos"]:
        assert sorted(info) == ["Alpha", "Eta", "GradNorm", "MeanKL"]
        assert info["GradNorm"].shape == (4,) and all(info[k].shape == (1,) for k in ("Alpha", "Eta", "MeanKL"))
        assert all(np.isfinite(v).all() for v in info.values()) and (info["GradNorm"] > 0).all()
        assert info["Eta"][0] >= 1e-8 and info["Alpha"][0] >= 1e-8
        assert info["Eta"][0] != F32(1.0) and info["Alpha"][0] != F32(5.0)
        assert info["MeanKL"][0] > 0                 # the call's last update sees parameters the first ones moved
    assert log["infos"][-1]["Eta"][0] == log["duals"][0] and log["infos"][-1]["Alpha"][0] == log["duals"][1]


def test_vmpo_trains_and_replayed_iterations_equal_eager_ones():
    """Six iterations: two eager, one captured, three replayed.  The same seeded run made eagerly ends in the same
    parameters and duals and returned the same diagnostics, bit for bit."""
    algo, policy, log = _train(True, 6)
    assert algo._graph is not None
    _assert_trained(algo, policy, log, 6)
    algo_e, policy_e, log_e = _train(False, 6)
    assert algo_e._graph is None
    _assert_same_run(log, policy, log_e, policy_e)
    assert np.array_equal(log["duals"], log_e["duals"])


def test_vmpo_trains_the_residual_network():
    algo, policy, log = _train(True, 4, resnet=True)
    assert algo._graph is not None and policy.n_params == 1164759
    _assert_trained(algo, policy, log, 4)
    algo_e, policy_e, log_e = _train(False, 4, resnet=True)
    assert algo_e._graph is None
    _assert_same_run(log, policy, log_e, policy_e)
    assert np.array_equal(log["duals"], log_e["duals"])


def test_the_weights_handed_to_the_head_are_the_restatement_s_selection():
    """One eager run, watched: at every minibatch the psi the head kernel reads is vmpo_ref's for that minibatch's idx
    under the eta of that moment -- the same selected set, values within one ulp, zero on the minibatch's other rows."""
    seen = []

    def wrap(algo, policy):
        inner = policy.loss_and_grads

        def watched(mb, kind, *a, **kw):
            assert kind == 4 and kw["duals"] is algo.optimizer.duals
            seen.append(dict(psi=mb["psi"].clone(), idx=mb["idx"].clone(), adv=mb["advantages"].clone(),
                             eta=kw["duals"][0:1].clone(), temp4=algo.optimizer.temp4.clone()))
            return inner(mb, kind, *a, **kw)
        policy.loss_and_grads = watched
    algo, policy, log = _train(False, 3, wrap=wrap)
    assert len(seen) == 12
    etas = set()
    for s in seen:
        idx = s["idx"].cpu().numpy().astype(np.int64)
        adv, psi, eta = s["adv"].cpu().numpy(), s["psi"].cpu().numpy(), float(s["eta"].item())
        etas.add(eta)
        assert idx.size == 20 and np.unique(idx).size == 20
        ref = vmpo_ref.weights(adv[idx], eta, algo.eps_eta)
        assert np.array_equal(psi[idx] > 0, ref["sel"]) and ref["n_top"] == 10
        assert within_one_ulp(psi[idx], ref["psi"].astype(F32)).all()
        assert s["temp4"][3].item() == 10
        assert abs(s["temp4"][1].item() - ref["d_eta"]) <= np.spacing(F32(max(ref["addends"][1], abs(ref["d_eta"]))))
    assert len(etas) == 12                           # eta moved at every update
