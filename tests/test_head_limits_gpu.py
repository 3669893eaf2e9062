"""The learners' output-stage kernels at the edges of what their entry points accept, against float64 restatements of
the reference's formulas, and the first value past each limit refused.

- policy-gradient head (csrc/learner.hip: arl_pg_head_infer / arl_pg_head_loss): 1 <= n_actions <= 18,
  1 <= hid <= 1024, any batch; the generic (any width) kernel next to the four specialised widths, the head gradient
  summed inside the head kernel (K * hid <= 3 072, K = n_actions + 1) and in the separate row-split kernel, splits
  that are empty (batch < 16) and long ones, and (18, 1024) at a batch where both kernels used to ask for more than
  64 KiB of dynamic LDS.  aac_base.py:60-70, a2c.py:43-46, ppo.py:42-51.
- C51 (csrc/dqn.hip: arl_catdqn_act / arl_catdqn_loss / arl_catdqn_loss_parts): 1 <= n_actions <= 64,
  2 <= n_atoms <= 64, any atom stride; dueling; shifted atoms on support points and outside the support; predicted
  probabilities below the 1e-6 clamp; 127 partial sums.  cat_dqn.py:40-109.
- DQN (arl_dqn_act / arl_dqn_loss): 1 <= n_actions <= 255; dueling; Huber at |delta| == delta_clip and one ulp either
  side.  dqn.py:137-172.

The references are tests/autograd_ref.ppo_surrogate, test_catdqn_gpu.ref_cat_loss and test_dqn_gpu.ref_q_loss run in
float64 on float64 copies of the fp32 inputs.  Tolerances scale with the reduction length (2e-5 sqrt(K) max|want|, as
test_noisy_net_gpu._tol).

Decisions that fp32 rounding could flip are kept away from their boundaries by construction, never decided in float64
near one: every PPO ratio sits a clear margin inside or outside the clip range, or is exactly 1 (old probability = the
kernel's own fp32 probability, so that s1 == s2 in both precisions and the tie goes to the first argument); every
greedy action wins by a clear margin (its top atom / its Q value is raised), except in deliberate exact ties (identical
rows, which stay identical through the dueling merge), where the first maximum wins in both precisions."""
import numpy as np
import pytest
import torch

import autograd_ref
from test_catdqn_gpu import ref_cat_loss
from test_dqn_gpu import ref_q_loss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _tol(want, k_red, scale=0.):
    return 2e-5 * np.sqrt(k_red) * max(want.abs().max().item(), scale, 1e-6)


def _close(got, want, k_red, what, scale=0.):
    """scale: a floor for max|want| where every entry can be far below its natural size (all rows saturated)."""
    err = (got.double() - want).abs().max().item() if want.numel() else 0.
    assert err <= _tol(want, k_red, scale), (what, err, _tol(want, k_red, scale))


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _untouched(t):
    return bool(torch.isnan(t).all())


def merge(val, adv):                     # dueling_merge_layer.py:32-35
    return val + (adv - adv.mean(dim=1, keepdim=True))


# ---------------------------------------------------------------------------------------------------- policy-gradient head

HEAD_CASES = [
    # (n_actions, hid, batch)
    (1, 1, 1), (2, 4, 3), (17, 60, 15), (18, 100, 16), (1, 128, 17), (18, 128, 1025),
    (2, 1000, 1025),                     # K * hid = 3 000: fused gradient, generic kernel
    (17, 1000, 3), (17, 1000, 4097),     # split kernel: empty splits; splits of 257 rows
    (5, 512, 4097), (6, 512, 15), (6, 512, 4097),      # just inside / just outside FUSED_WGRAD_MAX
    (1, 1024, 12288), (2, 60, 4097), (18, 1, 17), (17, 4, 16),
    (18, 1024, 1),                       # split kernel on one row, 77 824 B of head-kernel LDS
    (18, 1024, 12288),                   # both kernels' LDS past 64 KiB before the row chunking
    (6, 64, 5), (6, 256, 5),             # the two specialised widths (hid / 64 = 1, 4) no case above reaches
]


def _head_inputs(n_act, hid, batch, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    K, n_rows = n_act + 1, batch + 7
    h = torch.relu(torch.randn(batch, hid, device=DEV, generator=gen))
    w = torch.randn(K, hid, device=DEV, generator=gen) * (0.8 / np.sqrt(hid))
    b = torch.randn(K, device=DEV, generator=gen) * 0.1
    act = torch.randint(0, n_act, (n_rows,), device=DEV, generator=gen).to(torch.uint8)
    adv = torch.randn(n_rows, device=DEV, generator=gen)
    ret = torch.randn(n_rows, device=DEV, generator=gen)
    idx = torch.randperm(n_rows, device=DEV, generator=gen)[:batch].to(torch.int32)
    return gen, h, w, b, act, adv, ret, idx


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "A%d-hid%d-B%d" % c)
def test_pg_head_infer_vs_float64(L, case):
    n_act, hid, batch = case
    _, h, w, b, *_ = _head_inputs(n_act, hid, batch, 11 * hid + n_act + batch)
    prob, value = _nan(batch + 1, n_act), _nan(batch + 1)
    L.pg_head_infer(h, w, b, prob[:batch], value[:batch])
    out = h.double() @ w.double().t() + b.double()
    want_p, want_v = torch.softmax(out[:, :n_act], 1), out[:, n_act]
    _close(prob[:batch], want_p, hid, "prob")
    _close(value[:batch], want_v, hid, "value")
    assert _untouched(prob[batch]) and _untouched(value[batch:])


@pytest.mark.parametrize("kind", [0, 1], ids=["a2c", "ppo"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "A%d-hid%d-B%d" % c)
def test_pg_head_loss_vs_float64(L, case, kind):
    n_act, hid, batch = case
    K = n_act + 1
    masked = (n_act + hid + batch + kind) % 2 == 1
    mask_dh = batch % 2 == 1
    gen, h, w, b, act, adv, ret, idx = _head_inputs(n_act, hid, batch, 7 * hid + n_act + batch + kind)
    n_rows = adv.numel()
    sel = idx.long()
    rows = torch.arange(batch, device=DEV)
    a = act[sel].long()
    valids = None
    if masked:
        valids = (torch.rand(n_rows, device=DEV, generator=gen) < 0.7).to(torch.int8)
        valids[sel[0]] = 1
    lr_mult = torch.full((1,), 0.6, device=DEV)
    clip, c_v, c_e = 0.2, (0.25 if kind == 0 else 1.0), 0.01
    c_eff = float(np.float32(clip) * np.float32(0.6))          # the kernel's clip: clip_param * lr_mult in fp32
    # PPO's old probabilities: the kernel's own fp32 probability of the taken action divided by a ratio a clear margin
    # inside / outside [1 - c, 1 + c] = [0.88, 1.12], or exactly it (ratio 1, a tie of the two surrogates)
    old = torch.softmax(torch.randn(n_rows, n_act, device=DEV, generator=gen), 1)
    if kind == 1:
        p_k, v_k = torch.empty(batch, n_act, device=DEV), torch.empty(batch, device=DEV)
        L.pg_head_infer(h, w, b, p_k, v_k)
        pa_k = p_k[rows, a]
        r = torch.tensor([0.5, 0.95, 1.05, 2.0, 1.0], device=DEV)[torch.arange(batch, device=DEV) % 5]
        old[sel, a] = torch.where(r == 1., pa_k, pa_k / r)
        rk = (pa_k + np.float32(1e-8)) / (old[sel, a] + np.float32(1e-8))
        lo, hi = 1. - c_eff, 1. + c_eff
        assert bool((((rk - lo).abs() > 0.02) & ((rk - hi).abs() > 0.02)).all())
        assert bool((rk[r == 1.] == 1.).all())
    # ---- float64 reference
    h64, w64, b64 = (t.double().requires_grad_() for t in (h, w, b))
    out = h64 @ w64.t() + b64
    out.retain_grad()
    prob, value = torch.softmax(out[:, :n_act], 1), out[:, n_act]
    pa = prob[rows, a]
    if masked:
        vs = valids[sel].double()
        wgt, inv = vs / vs.sum(), (1. / valids[sel].sum(dtype=torch.float32)).reshape(1)
    else:
        wgt, inv = torch.full((batch,), 1. / batch, dtype=torch.float64, device=DEV), None
    adv_s, ret_s = adv[sel].double(), ret[sel].double()
    if kind == 1:
        ratio = (pa + 1e-8) / (old[sel, a].double() + 1e-8)
        pi_rows = wgt * autograd_ref.ppo_surrogate(ratio, adv_s, c_eff, "theano")
    else:
        pi_rows = wgt * torch.log(pa + 1e-8) * adv_s
    v_rows = c_v * wgt * (value - ret_s) ** 2
    e_rows = -c_e * wgt * -torch.sum(prob * torch.log(prob + 1e-8), dim=1)
    pi, vl, el = -pi_rows.sum(), v_rows.sum(), e_rows.sum()
    total = pi + vl + el
    g_out, g_h, g_w, g_b = torch.autograd.grad(total, [out, h64, w64, b64])
    if mask_dh:
        g_h = g_h * (h > 0)
    # ---- kernel, every output inside a larger NaN-filled buffer
    dout, dh = _nan(batch + 1, K), _nan(batch + 1, hid)
    dw, db, loss4 = _nan(K + 1, hid), _nan(K + 4), _nan(5)
    L.pg_head_loss(h, w, b, act, adv, ret, old, valids, idx, lr_mult, inv, n_act, kind, clip, c_v, c_e,
                   dout[:batch], dh[:batch], dw[:K], db[:K], loss4[:4], L.pg_head_workspace(DEV),
                   relu_mask_dh=mask_dh, tie_rule=L.PPO_TIE_THEANO)
    torch.cuda.synchronize()
    _close(dout[:batch], g_out, K, "dout")
    _close(dh[:batch], g_h, K, "dh")
    _close(dw[:K], g_w, batch, "dw")
    _close(db[:K], g_b, batch, "db")
    want4 = torch.stack([pi, vl, el, total]).detach()
    scale = [pi_rows.abs().sum(), v_rows.abs().sum(), e_rows.abs().sum()]
    scale.append(sum(scale))
    for i in range(4):                   # a sum over the batch: error relative to the sum of its terms' magnitudes
        err = abs(loss4[i].item() - want4[i].item())
        assert err <= 1e-5 * (scale[i].item() + 1.), (i, err, scale[i].item())
    assert _untouched(dout[batch]) and _untouched(dh[batch]) and _untouched(dw[K]) and _untouched(db[K:])
    assert _untouched(loss4[4:])


# ---------------------------------------------------------------------------------------------------- C51

V_MIN, V_MAX = -10., 10.
C51_SHAPES = [(1, 2), (2, 2), (64, 64), (61, 51), (64, 3)]


def _cat_select_logits(gen, batch, n_act, n_atoms, stride, dueling):
    """[B][A (+1)][stride] logits whose greedy action (first maximum of the expected Q, after the merge) wins by a clear
    margin, except rows 0 (every action identical: action 0) and 1 (the winner's row copied to a lower action: that
    one); padding columns poisoned.  Returns (logits, greedy action) -- the greedy action from float64, checked to be
    far from any fp32 tie."""
    rows = n_act + int(dueling)
    x = torch.randn(batch, rows, stride, device=DEV, generator=gen) * 2
    x[:, :, n_atoms:] = 1e9
    z64 = torch.linspace(V_MIN, V_MAX, n_atoms, device=DEV).double()

    def q_of(t):
        t = t[:, :, :n_atoms].double()
        if dueling:
            t = merge(t[:, n_act:], t[:, :n_act])
        return (torch.softmax(t, 2) * z64).sum(2)
    x[:, :, n_atoms - 1] -= 8.                                                # no action near Q = v_max ...
    win = torch.argmax(q_of(x), 1)
    x[torch.arange(batch, device=DEV), win, n_atoms - 1] += 25.               # ... but the winner: its top atom dominates
    if n_act > 1:
        x[0, 1:n_act] = x[0, 0]
        if batch > 1:
            w1 = int(torch.argmax(q_of(x[1:2]), 1))
            if w1 > 0:
                x[1, w1 // 2] = x[1, w1]
    q = q_of(x)
    greedy = torch.argmax(q, 1)
    if n_act > 1:
        top2 = torch.topk(q, 2, dim=1).values
        tie = top2[:, 0] == top2[:, 1]
        assert bool(((top2[:, 0] - top2[:, 1] > 1e-3) | tie).all())
        assert bool(tie[0]) and int(greedy[0]) == 0
    return x, greedy


@pytest.mark.parametrize("batch", [1, 5, 300])
@pytest.mark.parametrize("wide_stride", [False, True], ids=["stride4", "stride132"])
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("shape", C51_SHAPES, ids=lambda s: "A%d-n%d" % s)
def test_c51_loss_and_act_vs_float64(L, shape, dueling, wide_stride, batch):
    n_act, n_atoms = shape
    stride = 132 if wide_stride else (n_atoms + 3) // 4 * 4
    rows = n_act + int(dueling)
    double = batch != 5
    weighted = batch != 1
    gen = torch.Generator(device=DEV).manual_seed(1000 * n_act + 10 * n_atoms + stride + batch + int(dueling))
    z = torch.linspace(V_MIN, V_MAX, n_atoms, device=DEV)
    act = torch.randint(0, n_act, (batch,), device=DEV, generator=gen).to(torch.uint8)
    ret = torch.randn(batch, device=DEV, generator=gen) * 6                   # many shifted atoms clipped
    term = (torch.rand(batch, device=DEV, generator=gen) < 0.3).to(torch.uint8)
    # terminal rows whose return IS a support point, lies beyond either end, or is v_max exactly
    special = [z[n_atoms // 2].item(), V_MAX + 3., V_MIN - 3., V_MAX, z[1].item()]
    for i, v in enumerate(special[:batch]):
        ret[batch - 1 - i] = v
        term[batch - 1 - i] = 1
    isw = torch.rand(batch, device=DEV, generator=gen) + 0.1 if weighted else None
    gamma_n = float(np.float32(0.99 ** 3))
    pred = torch.randn(batch, rows, stride, device=DEV, generator=gen) * 2
    pred[:, :, n_atoms:] = 1e9
    # the taken action's logits (the value row under dueling) at +-40: most of its probabilities far below 1e-6
    sat = torch.arange(batch, device=DEV) % 3 == 0
    pm = torch.where(torch.arange(n_atoms, device=DEV) % 2 == 0, 40., -40.)
    bi = torch.arange(batch, device=DEV)[sat]
    pred[bi, act[sat].long(), :n_atoms] = pm
    if dueling:
        pred[bi, n_act, :n_atoms] = pm
    tgt, greedy_t = _cat_select_logits(gen, batch, n_act, n_atoms, stride, dueling)
    pol, greedy_p = _cat_select_logits(gen, batch, n_act, n_atoms, stride, dueling) if double else (None, None)
    # ---- kernel
    dl, lr, kl = _nan(batch + 1, rows, stride), _nan(batch + 1), _nan(batch + 1)
    L.catdqn_loss(pred, tgt, pol, z, act, ret, term, isw, n_act, n_atoms, V_MIN, V_MAX, gamma_n, dl[:batch],
                  lr[:batch], kl[:batch], dueling=dueling)
    torch.cuda.synchronize()
    # ---- float64 reference
    full = (lambda t: merge(t[:, n_act:], t[:, :n_act])) if dueling else (lambda t: t)      # noqa: E731
    p64 = pred[:, :, :n_atoms].double().requires_grad_()
    w64 = (isw.double() if weighted else torch.ones(batch, dtype=torch.float64, device=DEV)).requires_grad_()
    sl = lambda t: None if t is None else full(t[:, :, :n_atoms].double())                   # noqa: E731
    loss, kl_ref = ref_cat_loss(full(p64), sl(tgt), sl(pol), z.double(), act, ret.double(), term, w64, V_MIN, V_MAX,
                                gamma_n)
    g_p, g_w = torch.autograd.grad(loss, [p64, w64])
    rows_ref = (w64 * g_w).detach()                                            # isw_b loss_b / B
    ce = g_w.detach() * batch
    # |d loss / d logit| <= 2 isw / B; a row whose projection sits on clamped atoms has a tiny gradient, known only to the
    # projection's absolute rounding (~ eps isw / B)
    _close(dl[:batch, :, :n_atoms], g_p, n_atoms + n_act, "dlogits", scale=w64.max().item() / batch)
    assert not dl[:batch, :, n_atoms:].any(), "padding columns must be exactly 0"
    _close(lr[:batch], rows_ref, n_atoms, "loss_rows")
    kl_err = (kl[:batch].double() - kl_ref).abs().max().item()
    assert kl_err <= 2e-5 * np.sqrt(n_atoms) * (ce.abs().max().item() + kl_ref.abs().max().item() + 1.), kl_err
    assert _untouched(dl[batch]) and _untouched(lr[batch:]) and _untouched(kl[batch:])
    # ---- the action kernel on the same blocks: greedy = first maximum, override, one-hot rows
    for logits, want in ((tgt, greedy_t),) + (((pol, greedy_p),) if double else ()):
        ov = torch.full((batch,), -1, dtype=torch.int32, device=DEV)
        ov[2::4] = (torch.arange(len(ov[2::4]), device=DEV, dtype=torch.int32) * 7) % n_act
        onehot = _nan(batch + 1, n_act)
        greedy = torch.full((batch + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        L.catdqn_act(logits, z, ov, n_act, n_atoms, onehot[:batch], greedy[:batch], dueling=dueling)
        torch.cuda.synchronize()
        assert torch.equal(greedy[:batch].long(), want)
        chosen = torch.where(ov >= 0, ov.long(), want)
        assert torch.equal(onehot[:batch], torch.nn.functional.one_hot(chosen, n_act).float())
        assert _untouched(onehot[batch]) and greedy[batch].item() == 0xAB


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_c51_loss_parts_at_127_splits(L, dueling):
    """arl_catdqn_loss_parts at its last accepted split count (the run-time fold loop, 8 members in most fold groups) at
    64 actions x 64 atoms: bit for bit the loss of the folded logits, and that loss against float64."""
    n_act, n_atoms, batch, sp = 64, 64, 7, 127
    stride, rows = 64, n_act + int(dueling)
    r = rows * stride
    gen = torch.Generator(device=DEV).manual_seed(127 + int(dueling))
    srcs, folded, keep = [], [], []
    for _ in range(3):
        parts = torch.randn(sp, batch * r, device=DEV, generator=gen) * 0.2
        bias = torch.randn(r, device=DEV, generator=gen)
        out = torch.empty(batch * r, device=DEV)
        folds = L.FoldList()
        folds._n = 1
        it = folds._items[0]
        it.part, it.out, it.total, it.splits, it.valid = parts.data_ptr(), out.data_ptr(), batch * r, sp, 0
        folds.run()
        folded.append((out.view(batch, rows, stride) + bias.view(rows, stride)).contiguous())
        src = L.ArlLogitSrc()
        src.part, src.bias_or_null, src.split_stride, src.splits = parts.data_ptr(), bias.data_ptr(), batch * r, sp
        srcs.append(src)
        keep += [parts, bias]
    z = torch.linspace(V_MIN, V_MAX, n_atoms, device=DEV)
    act = torch.randint(0, n_act, (batch,), device=DEV, generator=gen).to(torch.uint8)
    ret = torch.randn(batch, device=DEV, generator=gen) * 6
    term = (torch.rand(batch, device=DEV, generator=gen) < 0.3).to(torch.uint8)
    isw = torch.rand(batch, device=DEV, generator=gen) + 0.1
    gamma_n = float(np.float32(0.99 ** 3))
    outs = []
    for parts_path in (False, True):
        dl, lr, kl = _nan(batch + 1, r), _nan(batch + 1), _nan(batch + 1)
        if parts_path:
            L.catdqn_loss_parts(srcs[0], srcs[1], srcs[2], z, act, ret, term, isw, n_act, n_atoms, stride, V_MIN,
                                V_MAX, gamma_n, dl[:batch], lr[:batch], kl[:batch], dueling=dueling)
        else:
            L.catdqn_loss(folded[0], folded[1], folded[2], z, act, ret, term, isw, n_act, n_atoms, V_MIN, V_MAX,
                          gamma_n, dl[:batch], lr[:batch], kl[:batch], dueling=dueling)
        torch.cuda.synchronize()
        assert _untouched(dl[batch]) and _untouched(lr[batch:]) and _untouched(kl[batch:])
        outs.append((dl[:batch], lr[:batch], kl[:batch]))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    # the folded logits' loss against float64: only where the greedy next action is clear of an fp32 tie
    full = (lambda t: merge(t[:, n_act:], t[:, :n_act])) if dueling else (lambda t: t)      # noqa: E731
    sl = lambda t: full(t.double())                                                        # noqa: E731
    q = (torch.softmax(sl(folded[2]), 2) * z.double()).sum(2)
    top2 = torch.topk(q, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert int(clear.sum()) >= batch - 2
    p64 = folded[0].double().requires_grad_()
    loss, kl_ref = ref_cat_loss(full(p64)[clear], sl(folded[1])[clear], sl(folded[2])[clear], z.double(),
                                act[clear], ret.double()[clear], term[clear], isw.double()[clear], V_MIN, V_MAX,
                                gamma_n)
    (g_p,) = torch.autograd.grad(loss * (int(clear.sum()) / batch), [p64])
    _close(outs[0][0].view(batch, rows, stride)[clear], g_p[clear], n_atoms + n_act, "dlogits")
    assert torch.allclose(outs[0][2][clear].double(), kl_ref, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- DQN

def _q_select_rows(gen, batch, n_act, stride, dueling):
    """[B][stride] Q rows (advantages + value column under dueling) whose first maximum after the merge wins by a clear
    margin, except row 0 (all advantages equal: action 0) and row 1 (the winner copied to a lower action); padding
    poisoned with 1e9."""
    q = torch.rand(batch, stride, device=DEV, generator=gen) * 2 - 1
    q[:, n_act + int(dueling):] = 1e9
    win = torch.randint(0, n_act, (batch,), device=DEV, generator=gen)
    q[torch.arange(batch, device=DEV), win] += 3.
    want = win.clone()
    if n_act > 1:
        q[0, 1:n_act] = q[0, 0]
        want[0] = 0
        if batch > 1 and int(win[1]) > 0:
            q[1, int(win[1]) // 2] = q[1, int(win[1])]
            want[1] = int(win[1]) // 2
    return q, want


def _q_merged(t, n_act, dueling):
    t = t.double()
    return merge(t[:, n_act:n_act + 1], t[:, :n_act]) if dueling else t[:, :n_act]


@pytest.mark.parametrize("double", [False, True], ids=["max", "double"])
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("n_act", [1, 2, 254, 255])
def test_dqn_loss_and_act_vs_float64(L, n_act, dueling, double):
    batch = 300
    stride = (n_act + int(dueling) + 4) // 4 * 4 + 4                       # > n_actions + 1, padding poisoned
    clip = 1.0 if double else float(np.float32(0.7))
    gen = torch.Generator(device=DEV).manual_seed(n_act * 4 + 2 * int(dueling) + int(double))
    q = torch.randn(batch, stride, device=DEV, generator=gen) * 2
    q[:, n_act + int(dueling):] = 1e9
    tgt, want_t = _q_select_rows(gen, batch, n_act, stride, dueling)
    pol, want_p = _q_select_rows(gen, batch, n_act, stride, dueling) if double else (None, None)
    act = torch.randint(0, n_act, (batch,), device=DEV, generator=gen).to(torch.uint8)
    ret = torch.randn(batch, device=DEV, generator=gen) * 2
    term = (torch.rand(batch, device=DEV, generator=gen) < 0.3).to(torch.uint8)
    isw = torch.rand(batch, device=DEV, generator=gen) + 0.1
    # Huber's boundary: terminal rows with Q == 0 (through the merge too), so delta = return exactly, and
    # weight isw / B = 2^-8 exactly, so that loss and gradient are known to the bit
    c32 = np.float32(clip)
    edge = [c32, np.nextafter(c32, np.float32(0)), np.nextafter(c32, np.float32(np.inf))]
    edge += [-e for e in edge]
    w_edge = np.float32(2. ** -8)
    for i, e in enumerate(edge):
        r = batch - 1 - i
        q[r, :n_act + int(dueling)] = 0.
        ret[r], term[r], isw[r] = float(e), 1, batch / 256.
    gamma_n = float(np.float32(0.99 ** 3))
    # ---- kernel
    dq, lr, td = _nan(batch + 1, stride), _nan(batch + 1), _nan(batch + 1)
    L.dqn_loss(q, tgt, pol, act, ret, term, isw, n_act, gamma_n, clip, dq[:batch], lr[:batch], td[:batch],
               dueling=dueling)
    torch.cuda.synchronize()
    # ---- float64 reference
    q64 = q.double().requires_grad_()
    w64 = isw.double().requires_grad_()
    loss, td_ref = ref_q_loss(_q_merged(q64, n_act, dueling), _q_merged(tgt, n_act, dueling),
                              None if pol is None else _q_merged(pol, n_act, dueling), act, ret.double(), term, w64,
                              gamma_n, clip)
    g_q, g_w = torch.autograd.grad(loss, [q64, w64])
    nv = n_act + int(dueling)
    _close(dq[:batch, :nv], g_q[:, :nv], n_act, "dq")
    assert not dq[:batch, nv:].any(), "padding columns must be exactly 0"
    _close(lr[:batch], (w64 * g_w).detach(), n_act, "loss_rows")
    _close(td[:batch], td_ref.detach(), n_act, "td_abs")
    # the boundary rows exactly: |delta| == clip and one ulp inside: squared branch; one ulp outside: Huber (equal
    # value and slope at the boundary, so both formulas give these numbers); priorities clipped to delta_clip
    for i, e in enumerate(edge):
        r = batch - 1 - i
        d = np.float32(e)
        ad = abs(d)
        slope = d if ad <= c32 else np.float32(np.copysign(c32, d))
        loss_r = np.float32(0.5) * (d * d) if ad <= c32 else c32 * (ad - c32 / np.float32(2))
        w = w_edge
        assert td[r].item() == float(min(ad, c32)), (i, td[r].item())
        assert lr[r].item() == float(w * loss_r), (i, lr[r].item(), float(w * loss_r))
        gq = -(w * slope)
        a_r = int(act[r])
        if not dueling:
            assert dq[r, a_r].item() == float(gq)
        else:
            assert dq[r, n_act].item() == float(gq)
            share = np.float32(gq) / np.float32(n_act)
            assert dq[r, a_r].item() == float(np.float32(gq) - share)
    assert _untouched(dq[batch]) and _untouched(lr[batch:]) and _untouched(td[batch:])
    # ---- the action kernel
    for rows_, want in ((tgt, want_t),) + (((pol, want_p),) if double else ()):
        ov = torch.full((batch,), -1, dtype=torch.int32, device=DEV)
        ov[3::5] = (torch.arange(len(ov[3::5]), device=DEV, dtype=torch.int32) * 13) % n_act
        onehot = _nan(batch + 1, n_act)
        greedy = torch.full((batch + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        L.dqn_act(rows_, ov, n_act, onehot[:batch], greedy[:batch], dueling=dueling)
        torch.cuda.synchronize()
        assert torch.equal(greedy[:batch].long(), want)
        assert torch.equal(greedy[:batch].long(), torch.argmax(_q_merged(rows_, n_act, dueling), 1))
        chosen = torch.where(ov >= 0, ov.long(), want)
        assert torch.equal(onehot[:batch], torch.nn.functional.one_hot(chosen, n_act).float())
        assert _untouched(onehot[batch]) and greedy[batch].item() == 0xAB


# ---------------------------------------------------------------------------------------------------- refusals

def _refused(call, match):
    """The entry point returns ARL_E_RANGE (-2, include/accel_rl_hip.h) with a message naming the limit."""
    with pytest.raises(RuntimeError, match=r"\(code -2\): .*" + match):
        call()


def test_pg_head_refuses_past_its_limits(L):
    batch = 8
    lib = L.load()
    h = torch.rand(batch, 1025, device=DEV)
    w, b = torch.rand(20, 1025, device=DEV), torch.rand(20, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    adv, ret = torch.rand(batch, device=DEV), torch.rand(batch, device=DEV)
    old, lr_mult = torch.rand(batch, 19, device=DEV), torch.ones(1, device=DEV)
    ws = L.pg_head_workspace(DEV)
    o = dict(prob=_nan(batch, 19), value=_nan(batch), dout=_nan(batch, 20), dh=_nan(batch, 1025), dw=_nan(20, 1025),
             db=_nan(20), loss4=_nan(4))
    p = {k: t.data_ptr() for k, t in o.items()}

    def infer(n, hid, n_act):            # the C entry points directly: a zero size has no tensor view with a pointer
        return L._check(lib.arl_pg_head_infer(h.data_ptr(), w.data_ptr(), b.data_ptr(), n, hid, n_act, p["prob"],
                                              p["value"], L.stream_ptr()), "arl_pg_head_infer")

    def loss(n, hid, n_act, kind):
        return L._check(lib.arl_pg_head_loss(
            h.data_ptr(), w.data_ptr(), b.data_ptr(), act.data_ptr(), adv.data_ptr(), ret.data_ptr(), old.data_ptr(),
            None, None, lr_mult.data_ptr(), None, n, hid, n_act, kind, L.PPO_TIE_THEANO, 0.2, 1., 0.01, 0, p["dout"],
            p["dh"], p["dw"], p["db"], p["loss4"], ws.data_ptr(), L.stream_ptr()), "arl_pg_head_loss")
    cases = ((batch, 64, 0, "n_actions <= 18"), (batch, 64, 19, "n_actions <= 18"), (batch, 0, 4, "hid <= 1024"),
             (batch, 1025, 4, "hid <= 1024"), (0, 64, 4, "batch"),
             (1 << 31, 64, 4, "batch <= 2\\^31"))      # rows are 32-bit indices in the kernels: refused before any read
    for n, hid, n_act, what in cases:
        _refused(lambda: infer(n, hid, n_act), what)
        for kind in (0, 1):
            _refused(lambda: loss(n, hid, n_act, kind), what)
    # the largest accepted sizes run (the float64 comparisons: test_pg_head_loss_vs_float64)
    infer(batch, 1024, 18)
    torch.cuda.synchronize()
    assert not torch.isnan(o["prob"].view(-1)[:batch * 18]).any()
    o["prob"].fill_(NAN)
    o["value"].fill_(NAN)
    for name, t in o.items():
        assert _untouched(t), name


def test_c51_refuses_past_its_limits(L):
    batch, stride = 4, 68
    lib = L.load()
    logits = torch.rand(batch, 66, stride, device=DEV)
    z = torch.linspace(-1, 1, 65, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret, term = torch.rand(batch, device=DEV), torch.zeros(batch, dtype=torch.uint8, device=DEV)
    onehot, greedy = _nan(batch, 66), torch.full((batch,), 0xAB, dtype=torch.uint8, device=DEV)
    dl, lr, kl = _nan(batch, 66, stride), _nan(batch), _nan(batch)

    def src(splits=1):
        s = L.ArlLogitSrc()
        s.part, s.bias_or_null, s.split_stride, s.splits = logits.data_ptr(), None, logits.numel(), splits
        return s
    for n_act, n_atoms, what in ((0, 51, "n_actions"), (65, 51, "n_actions <= 64"), (4, 1, "2 <= n_atoms"),
                                 (4, 65, "n_atoms <= 64")):
        for dueling in (0, 1):
            _refused(lambda: L._check(lib.arl_catdqn_act(logits.data_ptr(), z.data_ptr(), None, batch, n_act, n_atoms,
                                                         stride, dueling, onehot.data_ptr(), greedy.data_ptr(),
                                                         L.stream_ptr()), "arl_catdqn_act"), what)
            _refused(lambda: L._check(lib.arl_catdqn_loss(
                logits.data_ptr(), logits.data_ptr(), None, z.data_ptr(), act.data_ptr(), ret.data_ptr(),
                term.data_ptr(), None, batch, n_act, n_atoms, stride, dueling, -1., 1., 0.9, dl.data_ptr(),
                lr.data_ptr(), kl.data_ptr(), L.stream_ptr()), "arl_catdqn_loss"), what)
            _refused(lambda: L.catdqn_loss_parts(src(), src(), None, z, act, ret, term, None, n_act, n_atoms, stride,
                                                 -1., 1., 0.9, dl, lr, kl, dueling=bool(dueling)), what)
    # partial sums: 127 accepted (test_c51_loss_parts_at_127_splits), 128 refused
    _refused(lambda: L.catdqn_loss_parts(src(128), src(), None, z, act, ret, term, None, 4, 51, stride, -1., 1., 0.9,
                                         dl, lr, kl), "splits < 128")
    _refused(lambda: L.catdqn_loss_parts(src(), src(), src(128), z, act, ret, term, None, 4, 51, stride, -1., 1., 0.9,
                                         dl, lr, kl), "splits < 128")
    torch.cuda.synchronize()
    assert _untouched(onehot) and bool((greedy == 0xAB).all())
    assert _untouched(dl) and _untouched(lr) and _untouched(kl)


def test_dqn_refuses_past_its_limits(L):
    batch, stride = 4, 260
    q = torch.rand(batch, stride, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret, term = torch.rand(batch, device=DEV), torch.zeros(batch, dtype=torch.uint8, device=DEV)
    onehot, greedy = _nan(batch, 256), torch.full((batch,), 0xAB, dtype=torch.uint8, device=DEV)
    dq, lr, td = _nan(batch, stride), _nan(batch), _nan(batch)
    lib = L.load()
    for n_act in (0, 256):
        for dueling in (0, 1):
            _refused(lambda: L._check(lib.arl_dqn_act(q.data_ptr(), None, batch, n_act, stride, dueling,
                                                      onehot.data_ptr(), greedy.data_ptr(), L.stream_ptr()),
                                      "arl_dqn_act"), "n_actions <= 255")
            _refused(lambda: L.dqn_loss(q, q, None, act, ret, term, None, n_act, 0.9, 1., dq, lr, td,
                                        dueling=bool(dueling)), "n_actions <= 255")
    torch.cuda.synchronize()
    assert _untouched(onehot) and bool((greedy == 0xAB).all())
    assert _untouched(dq) and _untouched(lr) and _untouched(td)
