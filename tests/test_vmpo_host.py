"""V-MPO without a GPU: the float64 restatement of its device stages (tests/vmpo_ref.py) against autograd and at
hand-made selections, the algorithm's defaults and refusals, the three entry points' declarations and bindings, and the
compile of csrc/vmpo.hip for gfx950 with the compiler's resource report."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ppg_ref
import vmpo_ref
from conftest import ROOT

CASES = [(1, 1, 1), (2, 4, 3), (6, 16, 9), (18, 8, 5)]          # (n_actions, hid, batch)


def _inputs(n_act, hid, batch, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                          # noqa: E731
    h = torch.relu(r(batch, hid)) + 0.01
    w, b = r(n_act + 1, hid) * (0.8 / np.sqrt(hid)), r(n_act + 1) * 0.1
    act = torch.randint(0, n_act, (batch,), generator=g)
    old = torch.softmax(r(batch, n_act), dim=1)
    old[0, 0] = 0.                                         # an exact zero (TINY at work)
    wgt = torch.full((batch,), 1. / batch, dtype=torch.float64)
    adv = r(batch).float().numpy()
    psi = torch.from_numpy(vmpo_ref.weights(adv, 0.7, 0.01)["psi"])
    return h, w, b, act, psi, r(batch), old, wgt


@pytest.mark.parametrize("case", CASES, ids=lambda c: "A%d-hid%d-B%d" % c)
def test_head_closed_form_equals_autograd_with_psi_and_alpha_detached(case):
    n_act, hid, batch = case
    h, w, b, act, psi, ret, old, wgt = _inputs(n_act, hid, batch, 5 * hid + n_act + batch)
    alpha, c_v = 3.5, 0.5
    hg, wg, bg = (t.clone().requires_grad_() for t in (h, w, b))
    prob, value, out = ppg_ref.head(hg, wg, bg, n_act)
    pi, v, akl, _ = vmpo_ref.losses(prob, value, act, psi, ret, old, alpha, c_v, wgt)
    g_out, g_h, g_w, g_b = torch.autograd.grad(pi + v + akl, [out, hg, wg, bg])
    with torch.no_grad():
        dout = vmpo_ref.dout(prob, value, act, psi, ret, old, alpha, c_v, wgt)
        dh, dw, db = ppg_ref.head_grads(dout, h, w, n_act, stop_value=False)
    for got, want in ((dout, g_out), (dh, g_h), (dw, g_w), (db, g_b)):
        assert (got - want).abs().max().item() <= 1e-13 * max(want.abs().max().item(), 1.)
    assert dout[:, n_act].abs().max() > 0                    # the value gradient is there and reaches dh
    # old == prob, psi == 0: the KL term and its gradient vanish up to TINY
    with torch.no_grad():
        zero = torch.zeros_like(psi)
        _, _, _, kl = vmpo_ref.losses(prob, value, act, zero, ret, prob, alpha, c_v, wgt)
        d0 = vmpo_ref.dout(prob, value, act, zero, ret, prob, alpha, c_v, wgt)
    assert abs(kl.item()) <= 1e-12 and d0[:, :n_act].abs().max().item() <= 1e-6 * alpha / batch


@pytest.mark.parametrize("n,eta", [(1, 1.0), (2, 0.3), (3, 2.0), (9, 0.7), (64, 0.05), (257, 1.0)])
def test_temperature_terms_equal_autograd_over_the_selected_rows(n, eta):
    adv = np.random.RandomState(n).randn(n).astype(np.float32)
    eps_eta = 0.01
    ref = vmpo_ref.weights(adv, eta, eps_eta)
    eta_t = torch.tensor(float(np.float32(eta)), dtype=torch.float64, requires_grad=True)
    sel_adv = torch.from_numpy(adv.astype(np.float64)[ref["sel"]])
    loss = vmpo_ref.temp_loss_sym(sel_adv, eta_t, eps_eta)
    (g,) = torch.autograd.grad(loss, [eta_t])
    assert abs(ref["temp_loss"] - loss.item()) <= 1e-13 * max(abs(loss.item()), 1.)
    assert abs(ref["d_eta"] - g.item()) <= 1e-13 * max(abs(g.item()), ref["addends"][1], 1.)
    assert abs(ref["psi"].sum() - 1.) <= 1e-15 * n and not ref["psi"][~ref["sel"]].any()
    assert ref["n_top"] == (n + 1) // 2 and (ref["psi"][ref["sel"]] > 0).all()


def test_selection_at_hand_made_cases():
    f = lambda *x: np.array(x, dtype=np.float32)                                               # noqa: E731
    sel = lambda *x: vmpo_ref.select(f(*x)).tolist()                                           # noqa: E731
    # all equal: the first n_top positions
    assert sel(2., 2., 2., 2., 2.) == [True, True, True, False, False]
    assert sel(-1., -1., -1., -1.) == [True, True, False, False]
    # a tie block straddling the threshold: 5 > the block of 1s; two places are left for the first two of its four
    assert sel(1., 0., 1., 5., 1., 1., -3.) == [True, False, True, True, True, False, False]
    assert sel(1., 1., 3., 1., 3., 1.) == [True, False, True, False, True, False]
    # +0.0 before -0.0, whatever the positions
    assert sel(-0., 0.) == [False, True] and sel(0., -0.) == [True, False]
    assert sel(-0., -0., 0., 0.) == [False, False, True, True]
    assert sel(-0., 0., -0., -1.) == [True, True, False, False]
    # n = 1, 2, 3
    assert sel(-7.) == [True] and sel(1., 2.) == [False, True] and sel(1., 1.) == [True, False]
    assert sel(1., 3., 2.) == [False, True, True] and sel(3., 3., 3.) == [True, True, False]
    # the keys order every fp32 value the way the values are ordered
    v = f(-np.inf, -3e38, -1., -1e-45, -0., 0., 1e-45, 1., 3e38, np.inf)
    k = vmpo_ref.keys(v).astype(np.int64)
    assert (np.diff(k) > 0).all()
    for n in (1, 2, 3, 10, 11):
        adv = np.random.RandomState(n).randn(n).astype(np.float32)
        ref = vmpo_ref.weights(adv, 1.0, 0.01)
        assert ref["sel"].sum() == (n + 1) // 2 and adv[ref["sel"]].min() >= np.sort(adv)[n // 2]
        assert abs(ref["psi"].sum() - 1.) <= 1e-15 * n and not ref["psi"][~ref["sel"]].any()


# ---- the algorithm -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs,match", [
    (dict(eps_eta=-0.1), "eps_eta"), (dict(eps_eta=float("nan")), "eps_eta"), (dict(eps_alpha=float("inf")), "eps_alpha"),
    (dict(eps_alpha="1"), "eps_alpha"), (dict(eta_init=0.), "eta_init"), (dict(eta_init=float("nan")), "eta_init"),
    (dict(alpha_init=-1.), "alpha_init"), (dict(alpha_init=True), "alpha_init"),
    (dict(v_loss_coeff=float("inf")), "v_loss_coeff"), (dict(discount=1.5), "discount"), (dict(gae_lambda=-0.1), "gae_lambda"),
    (dict(optimizer_args=dict(epochs=0)), "epochs"), (dict(optimizer_args=dict(minibatch_size=0)), "minibatch_size"),
    (dict(optimizer_args=dict(minibatch_size="third")), "minibatch_size"),
    (dict(optimizer_args=dict(dual_args=dict(momentum=1))), "dual_args"), (dict(lr_schedule="cosine"), "lr_schedule")])
def test_constructor_refusals(kwargs, match):
    from accel_rl_amd.algos.pg import VMPO
    with pytest.raises(ValueError, match=match):
        VMPO(**kwargs)


class _Policy(object):
    recurrent = False


def test_defaults_and_initialize_refusals():
    from accel_rl_amd import _lib
    from accel_rl_amd.algos.pg import VMPO
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.single import PpoOptimizer, VmpoOptimizer
    algo = VMPO()
    assert (algo.eps_eta, algo.eps_alpha, algo.eta_init, algo.alpha_init) == (0.01, 0.005, 1.0, 5.0)
    assert (algo.v_loss_coeff, algo.discount, algo.gae_lambda, algo.ent_loss_coeff) == (0.5, 0.99, 1, 0.)
    assert algo.loss_kind == 4 and algo.standardize_adv is False and algo.use_graph
    opt = algo.optimizer
    assert isinstance(opt, VmpoOptimizer) and issubclass(VmpoOptimizer, PpoOptimizer)
    assert opt._epochs == 4 and opt._update_method.name == "adam" and opt._learning_rate == 1e-4
    assert opt._grad_norm_clip is None and opt.dual_init == (1.0, 5.0) and opt.eps_alpha == 0.005
    assert (opt._dual_lr, opt._dual_method.name, opt._dual_kernel_args) == (1e-4, "adam", (0.9, 0.999, 1e-8))
    assert algo.opt_info_keys == ["GradNorm", "Eta", "Alpha", "MeanKL"]
    # the duals' optimiser: the network's unless dual_args says otherwise
    o = VMPO(optimizer_args=dict(update_method_args=dict(epsilon=1e-5),
                                 dual_args=dict(learning_rate=3e-3))).optimizer
    assert (o._dual_lr, o._dual_kernel_args) == (3e-3, (0.9, 0.999, 1e-5))
    o = VMPO(optimizer_args=dict(dual_args=dict(update_method=update_methods.rmsprop))).optimizer
    assert (o._dual_method.name, o._dual_kernel_args, o._update_method.name) == ("rmsprop", (0.9, 0.0, 1e-6), "adam")

    class Recurrent(_Policy):
        recurrent = True

    class Sync(VmpoOptimizer):
        parallelism_tag = "synchronous"
    with pytest.raises(NotImplementedError, match="recurrent"):
        VMPO().initialize(Recurrent(), None, 40, 5, True)
    with pytest.raises(NotImplementedError, match="mid_batch_reset=False"):
        VMPO().initialize(_Policy(), None, 40, 5, False)
    with pytest.raises(NotImplementedError, match="single GPU only"):
        VMPO(OptimizerCls=Sync).initialize(_Policy(), None, 40, 5, True)
    with pytest.raises(ValueError, match=r"minibatches of %d rows" % (_lib.VMPO_MAX_ROWS + 1)):
        VMPO(optimizer_args=dict(minibatch_size=None)).initialize(_Policy(), None, _lib.VMPO_MAX_ROWS + 1, 1, True)
    # 4 epochs x (40 // 2 = 20) = 80 updates: more than one optimizer call logs
    with pytest.raises(ValueError, match=r"= 80 updates"):
        VMPO(optimizer_args=dict(minibatch_size=2)).initialize(_Policy(), None, 40, 5, True)
    with pytest.raises(ValueError, match=r"= 0 updates"):
        VMPO(optimizer_args=dict(minibatch_size=41)).initialize(_Policy(), None, 40, 5, True)


def test_pi_loss_is_the_weighted_log_likelihood():
    from accel_rl_amd.algos.pg import VMPO
    from accel_rl_amd.distributions import Categorical
    policy = _Policy()
    policy.distribution = Categorical(3)
    prob = torch.tensor([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3]], dtype=torch.float64)
    act, psi = torch.tensor([2, 0]), torch.tensor([0.25, 0.75], dtype=torch.float64)
    got = VMPO().pi_loss(policy, act, psi, None, dict(prob=prob), None)
    want = -(0.25 * np.log(0.5 + 1e-8) + 0.75 * np.log(0.6 + 1e-8))
    assert abs(got.item() - want) <= 1e-15
    with pytest.raises(NotImplementedError, match="valids"):
        VMPO().pi_loss(policy, act, psi, None, dict(prob=prob), torch.ones(2))


# ---- the entry points ----------------------------------------------------------------------------------------------------

ENTRIES = dict(arl_vmpo_weights=8, arl_vmpo_head_loss_parts=23, arl_vmpo_dual_step=14)


def test_entries_are_declared_and_bound_with_matching_arguments():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    assert lib.arl_abi_version() == 5 and _lib.ARL_ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "accel_rl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}
    for name, count in ENTRIES.items():
        (decl,) = re.findall(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        params = [p.split() for p in decl.split(",")]
        res, argtypes = _lib._SIGNATURES[name]
        assert len(params) == len(argtypes) == count and name in _lib.EXPORTED_SYMBOLS and res is ctypes.c_int32
        for p, t in zip(params, argtypes):                   # pointers, integers and floats sit where the header has them
            want = ctypes.c_void_p if "*" in " ".join(p) else kinds[p[0]]
            assert t is want, (name, p, t)
        assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None
    (rows,) = re.findall(r"#define\s+ARL_VMPO_MAX_ROWS\s+(\d+)\b", text)
    assert int(rows) == _lib.VMPO_MAX_ROWS == 65536
    assert "vmpo.hip" in _build.SOURCES
    assert hasattr(_lib.FoldList, "vmpo_head_loss") and callable(_lib.vmpo_weights) and callable(_lib.vmpo_dual_step)


def test_argument_errors_come_back_before_any_launch():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                # (never dereferenced: every call below is refused)
    assert lib.arl_vmpo_weights(None, None, 4, None, 0.01, None, None, None) == -1 and b"null" in lib.arl_last_error()
    for n in (0, -1, 65537):
        assert lib.arl_vmpo_weights(one, None, n, one, 0.01, one, one, None) == -2
        assert b"ARL_VMPO_MAX_ROWS" in lib.arl_last_error()
    assert lib.arl_vmpo_weights(one, None, 4, one, float("nan"), one, one, None) == -1
    assert b"eps_eta" in lib.arl_last_error()
    head = [None] * 10 + [1, 1, 1, 0.5, 0] + [None] * 8
    assert lib.arl_vmpo_head_loss_parts(*head) == -1 and b"null" in lib.arl_last_error()
    full = [one] * 10 + [1, 1, 1, 0.5, 0] + [one] * 7 + [None]
    for pos in (0, 1, 2, 3, 4, 5, 6, 8, 15, 16, 17, 18, 19, 20, 21):           # every pointer but idx and inv_count
        args = list(full)
        args[pos] = None
        assert lib.arl_vmpo_head_loss_parts(*args) == -1 and b"null" in lib.arl_last_error(), pos
    for bad in (float("nan"), float("inf")):
        args = list(full)
        args[13] = bad
        assert lib.arl_vmpo_head_loss_parts(*args) == -1 and b"v_loss_coeff" in lib.arl_last_error()
    for kw in ({10: 0}, {10: 1 << 31}, {11: 0}, {11: 1025}, {12: 0}, {12: 19}):
        args = list(full)
        for k, v in kw.items():
            args[k] = v
        assert lib.arl_vmpo_head_loss_parts(*args) == -2, kw
    dual = [one] * 7 + [0.005, 0, 1e-4, 0.9, 0.999, 1e-8, None]
    assert lib.arl_vmpo_dual_step(*([None] * 7 + dual[7:])) == -1 and b"null" in lib.arl_last_error()
    for pos in (0, 1, 3, 4, 5, 6):
        args = list(dual)
        args[pos] = None
        assert lib.arl_vmpo_dual_step(*args) == -1, pos
    args = list(dual)
    args[2] = None                                           # adam needs slot1; rmsprop does not read it
    assert lib.arl_vmpo_dual_step(*args) == -1 and b"slot1" in lib.arl_last_error()
    for kw, code in (({8: 2}, -1), ({7: float("nan")}, -1), ({10: 1.0}, -2), ({11: -0.1}, -2), ({12: -1e-8}, -2),
                     ({9: float("nan")}, -2), ({8: 1, 10: 1.5}, -2)):
        args = list(dual)
        for k, v in kw.items():
            args[k] = v
        assert lib.arl_vmpo_dual_step(*args) == code, kw


def test_vmpo_kernels_compile_for_gfx950_without_scratch():
    """The compiler's own report (-Rpass-analysis=kernel-resource-usage), printed, for csrc/vmpo.hip: every head_kernel
    variant of VmpoLoss keeps its per-action values in registers (scratch 0) within the 128 VGPRs that leave four waves
    per SIMD; the weights kernel (one workgroup of 1 024: at most 128 VGPRs too) and the dual kernels have no scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    field = lambda name, block: int(re.search(name + r": (\d+)", block).group(1))             # noqa: E731
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "accel_rl_amd", "csrc"),
                          "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "accel_rl_amd", "csrc", "vmpo.hip"), "-o", os.devnull],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    blocks = out.split("Function Name: ")[1:]
    count = lambda piece: sum(piece in b.split()[0] for b in blocks)                            # noqa: E731
    assert count("head_wgrad_kernel") == 1 and count("11head_kernelI") == 5 and count("8VmpoLossE") == 5
    assert count("vmpo_weights_kernel") == 1 and count("vmpo_dual_kernel") == 2 and len(blocks) == 9
    for b in blocks:
        name = b.split()[0]
        vgprs, scratch = field("VGPRs", b), field(r"ScratchSize \[bytes/lane\]", b)
        print("%-80s VGPRs %3d SGPRs %3d scratch %d LDS %d occupancy %d" % (
            name, vgprs, field("TotalSGPRs", b), scratch, field(r"LDS Size \[bytes/block\]", b),
            field(r"Occupancy \[waves/SIMD\]", b)))
        assert scratch == 0 and vgprs <= 128, name
