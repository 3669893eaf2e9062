"""PPG without a GPU: the float64 restatement of its two output stages (tests/ppg_ref.py) against autograd, the
algorithm's refusals, the new entry point's declaration and binding, and the compile for gfx950 of the two files that instantiate
the head kernel (learner.hip, ppg.hip) with the compiler's resource report."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ppg_ref
from conftest import ROOT

CASES = [(1, 1, 1), (2, 4, 3), (6, 16, 9), (18, 8, 5)]          # (n_actions, hid, batch)


def _inputs(n_act, hid, batch, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                          # noqa: E731
    h = torch.relu(r(batch, hid)) + 0.01
    w, b = r(n_act + 1, hid) * (0.8 / np.sqrt(hid)), r(n_act + 1) * 0.1
    act = torch.randint(0, n_act, (batch,), generator=g)
    old = torch.softmax(r(batch, n_act), dim=1)
    old[0, 0] = 0.                                         # an exact zero (the auxiliary phase's TINY at work)
    wgt = torch.full((batch,), 1. / batch, dtype=torch.float64)
    return h, w, b, act, r(batch), r(batch), old, wgt


@pytest.mark.parametrize("tie_rule", ["theano", "math", "both"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "A%d-hid%d-B%d" % c)
def test_policy_phase_closed_form_equals_autograd_with_the_value_path_detached(case, tie_rule):
    n_act, hid, batch = case
    h, w, b, act, adv, ret, old, wgt = _inputs(n_act, hid, batch, 3 * hid + n_act + batch)
    with torch.no_grad():
        prob0, _, _ = ppg_ref.head(h, w, b, n_act)
        pa0 = prob0[torch.arange(batch), act]
        # ratios 0.5 / 0.95 / 1.05 / 2 / exactly 1 by rows: outside, inside and on the tie of the two surrogates
        r = torch.tensor([0.5, 0.95, 1.05, 2.0, 1.0], dtype=torch.float64)[torch.arange(batch) % 5]
        old_pa = torch.where(r == 1., pa0, (pa0 + ppg_ref.TINY) / r - ppg_ref.TINY)
    clip, c_v, c_e = 0.12, 0.5, 0.01
    hg, wg, bg = (t.clone().requires_grad_() for t in (h, w, b))
    prob, value, out = ppg_ref.head(hg, wg, bg, n_act, stop_value=True)
    out.retain_grad()
    total = sum(ppg_ref.policy_losses(prob, value, act, adv, ret, old_pa, clip, c_v, c_e, wgt, tie_rule))
    g_h, g_w, g_b = torch.autograd.grad(total, [hg, wg, bg], retain_graph=True)
    (g_out,) = torch.autograd.grad(total, [out])
    with torch.no_grad():
        dout = ppg_ref.policy_dout(prob, value, act, adv, ret, old_pa, clip, c_v, c_e, wgt, tie_rule)
        dh, dw, db = ppg_ref.head_grads(dout, h, w, n_act, stop_value=True)
    for got, want in ((dout, g_out), (dh, g_h), (dw, g_w), (db, g_b)):
        assert (got - want).abs().max().item() <= 1e-13 * max(want.abs().max().item(), 1.)
    assert dout[:, n_act].abs().max() > 0                    # the value loss is there, and only the head sees it


@pytest.mark.parametrize("case", CASES, ids=lambda c: "A%d-hid%d-B%d" % c)
def test_auxiliary_phase_closed_form_equals_autograd(case):
    n_act, hid, batch = case
    h, w, b, _, _, ret, old, wgt = _inputs(n_act, hid, batch, 5 * hid + n_act + batch)
    beta, c_v = 0.7, 0.5
    hg, wg, bg = (t.clone().requires_grad_() for t in (h, w, b))
    prob, value, out = ppg_ref.head(hg, wg, bg, n_act)
    total = sum(ppg_ref.aux_losses(prob, value, ret, old, beta, c_v, wgt))
    g_out, g_h, g_w, g_b = torch.autograd.grad(total, [out, hg, wg, bg])
    with torch.no_grad():
        dout = ppg_ref.aux_dout(prob, value, ret, old, beta, c_v, wgt)
        dh, dw, db = ppg_ref.head_grads(dout, h, w, n_act, stop_value=False)
    for got, want in ((dout, g_out), (dh, g_h), (dw, g_w), (db, g_b)):
        assert (got - want).abs().max().item() <= 1e-13 * max(want.abs().max().item(), 1.)
    # old == prob: the clone term and its gradient vanish up to TINY
    with torch.no_grad():
        clone, _ = ppg_ref.aux_losses(prob, value, ret, prob, beta, c_v, wgt)
        d0 = ppg_ref.aux_dout(prob, value, ret, prob, beta, c_v, wgt)
    assert abs(clone.item()) <= 1e-12 and d0[:, :n_act].abs().max().item() <= 1e-6 * beta / batch


def test_stopped_gradient_is_the_composition_the_gpu_tests_use():
    """Below the head, grad(pi + v + ent) with the value path detached equals grad(pi + ent); for the head's two tensors
    it is that plus grad(v) with respect to them alone."""
    n_act, hid, batch = 4, 8, 6
    h0, w, b, act, adv, ret, old, wgt = _inputs(n_act, hid, batch, 77)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(batch, 5, generator=g, dtype=torch.float64)
    w1 = torch.randn(5, hid, generator=g, dtype=torch.float64).requires_grad_()
    wg, bg = w.clone().requires_grad_(), b.clone().requires_grad_()
    old_pa = old[torch.arange(batch), act] + 0.05
    args = (act, adv, ret, old_pa, 0.2, 0.5, 0.01, wgt)
    prob, value, _ = ppg_ref.head(torch.relu(x @ w1), wg, bg, n_act, stop_value=True)
    stopped = torch.autograd.grad(sum(ppg_ref.policy_losses(prob, value, *args)), [w1, wg, bg])
    prob, value, _ = ppg_ref.head(torch.relu(x @ w1), wg, bg, n_act)
    pi, v, ent = ppg_ref.policy_losses(prob, value, *args)
    trunk = torch.autograd.grad(pi + ent, [w1, wg, bg], retain_graph=True)
    head_v = torch.autograd.grad(v, [wg, bg])
    composed = [trunk[0], trunk[1] + head_v[0], trunk[2] + head_v[1]]
    for got, want in zip(composed, stopped):
        assert (got - want).abs().max().item() <= 1e-14 * max(want.abs().max().item(), 1.)


# ---- the algorithm's refusals ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs,match", [
    (dict(n_pi=0), "n_pi"), (dict(n_pi=2.0), "n_pi"), (dict(n_pi=True), "n_pi"), (dict(e_aux=0), "e_aux"),
    (dict(e_aux="6"), "e_aux"), (dict(beta_clone=-0.1), "beta_clone"), (dict(beta_clone=float("nan")), "beta_clone"),
    (dict(aux_v_loss_coeff=float("inf")), "aux_v_loss_coeff"), (dict(aux_v_loss_coeff=-1), "aux_v_loss_coeff"),
    (dict(aux_optimizer_args=dict(epochs=3)), "e_aux"), (dict(aux_minibatch_size=0), "aux_minibatch_size")])
def test_constructor_refusals(kwargs, match):
    from accel_rl_amd.algos.pg import PPG
    with pytest.raises(ValueError, match=match):
        PPG(**kwargs)


class _Policy(object):
    recurrent = False

    def prob_value_rows(self):
        pass


def test_defaults_and_initialize_refusals():
    from accel_rl_amd.algos.pg import PPG
    from accel_rl_amd.optimizers.single import PpoOptimizer
    algo = PPG()
    assert (algo.n_pi, algo.e_aux, algo.beta_clone, algo.aux_v_loss_coeff) == (32, 6, 1.0, 0.5)
    assert (algo.clip_param, algo.ent_loss_coeff, algo.v_loss_coeff, algo.gae_lambda) == (0.2, 0.01, 0.5, 0.95)
    assert algo.optimizer._epochs == 1 and algo.optimizer._update_method.name == "adam" and algo.loss_kind == 2
    assert algo.opt_info_keys == ["GradNorm", "AuxVLoss", "AuxCloneLoss"]

    class Recurrent(_Policy):
        recurrent = True

    class NoRows(object):
        recurrent = False

    class Sync(PpoOptimizer):
        parallelism_tag = "synchronous"
    with pytest.raises(NotImplementedError, match="recurrent"):
        PPG().initialize(Recurrent(), None, 40, 5, True)
    with pytest.raises(NotImplementedError, match="mid_batch_reset=False"):
        PPG().initialize(_Policy(), None, 40, 5, False)
    with pytest.raises(NotImplementedError, match="single GPU only"):
        PPG(OptimizerCls=Sync).initialize(_Policy(), None, 40, 5, True)
    with pytest.raises(TypeError, match="prob_value_rows"):
        PPG().initialize(NoRows(), None, 40, 5, True)
    # 6 epochs x (1280 // 100 = 12) = 72 updates: more than one optimizer call logs
    with pytest.raises(ValueError, match=r"= 72 updates"):
        PPG(aux_minibatch_size=100).initialize(_Policy(), None, 40, 5, True)
    with pytest.raises(ValueError, match=r"= 0 updates"):
        PPG(n_pi=1, aux_minibatch_size=41).initialize(_Policy(), None, 40, 5, True)


# ---- the entry point ----------------------------------------------------------------------------------------------------

def test_entry_is_declared_and_bound_with_matching_arguments():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    assert lib.arl_abi_version() == 5 and _lib.ARL_ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "accel_rl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    (decl,) = re.findall(r"\bint\s+arl_ppg_head_loss_parts\s*\(([^)]*)\)\s*;", text)
    params = [p.split() for p in decl.split(",")]
    res, argtypes = _lib._SIGNATURES["arl_ppg_head_loss_parts"]
    assert len(params) == len(argtypes) == 28 and "arl_ppg_head_loss_parts" in _lib.EXPORTED_SYMBOLS
    import ctypes
    for p, t in zip(params, argtypes):                       # pointers, integers and floats sit where the header has them
        want = (ctypes.c_void_p if "*" in " ".join(p) else
                {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}[p[0]])
        assert t is want, (p, t)
    assert re.search(r"#define\s+ARL_PPG_POLICY\s+0\b", text) and re.search(r"#define\s+ARL_PPG_AUX\s+1\b", text)
    assert (_lib.PPG_POLICY, _lib.PPG_AUX) == (0, 1)
    assert "ppg.hip" in _build.SOURCES
    # argument errors come back before any HIP call
    null = [None] * 10 + [1, 1, 1, 0, 0, 0.2, 0.5, 0.01, 1.0, 0] + [None] * 8
    assert lib.arl_ppg_head_loss_parts(*null) == -1 and b"null" in lib.arl_last_error()
    null[13] = 2
    assert lib.arl_ppg_head_loss_parts(*null) == -1 and b"phase" in lib.arl_last_error()


def test_head_kernels_compile_for_gfx950_without_scratch():
    """The compiler's own report (-Rpass-analysis=kernel-resource-usage), printed, for both files that instantiate
    head_kernel_dev.h's kernel: every head_kernel variant keeps its per-action values in registers (scratch 0) and within
    the 128 VGPRs that leave four waves per SIMD, and so does each file's head_wgrad_kernel."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    field = lambda name, block: int(re.search(name + r": (\d+)", block).group(1))             # noqa: E731
    for source, losses in (("learner.hip", ["InferLoss", "PgLoss"]), ("ppg.hip", ["PpgPolicyLoss", "PpgAuxLoss"])):
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                              "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "accel_rl_amd", "csrc"),
                              "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                              os.path.join(ROOT, "accel_rl_amd", "csrc", source), "-o", os.devnull],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
        blocks = [b for b in out.split("Function Name: ")[1:] if "head_" in b.split()[0]]
        # mangled names: head_kernel<Loss, HVT> carries "11head_kernelI" and the loss's name; one variant per width
        count = lambda piece: sum(piece in b.split()[0] for b in blocks)                        # noqa: E731
        assert count("head_wgrad_kernel") == 1 and count("11head_kernelI") == 10 and len(blocks) == 11, source
        for loss in losses:
            assert count("%d%sE" % (len(loss), loss)) == 5, loss   # 4 specialised widths + the generic one
        for b in blocks:
            vgprs, scratch = field("VGPRs", b), field(r"ScratchSize \[bytes/lane\]", b)
            print("%-80s VGPRs %3d SGPRs %3d scratch %d LDS %d occupancy %d" % (
                b.split()[0], vgprs, field("TotalSGPRs", b), scratch, field(r"LDS Size \[bytes/block\]", b),
                field(r"Occupancy \[waves/SIMD\]", b)))
            assert scratch == 0 and vgprs <= 128
