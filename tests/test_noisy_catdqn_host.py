"""CPU-only checks of the noisy categorical DQN policy and Rainbow (accel_rl_amd/policies/dqn/
atari_noisy_net_cat_dqn_policy.py, accel_rl_amd/algos/dqn/rainbow.py): the constructor's refusals, the reference's
parameter names, shapes and initial draw order (the bucket lives on the host here), argument errors of the new entry
points without a GPU, the new ABI structs' layouts against gcc, and Rainbow's defaults and policy checks."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT


def _spec(no=0, **kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    spec = dict(cnn_specs[no])
    spec.update(kw)
    return spec


def _host_policy(dueling, seed=11, n_act=6, **kw):
    from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(seed)
    p = AtariNoisyNetCatDqnPolicy(dueling=dueling, **_spec(**kw))
    p.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device="cpu")
    return p


def test_constructor_refusals():
    from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    for kw in (dict(factorized=False), dict(n_atoms=1), dict(n_atoms=65), dict(dueling=True, hidden_sizes=(256, 256)),
               dict(dueling=True, hidden_sizes=()), dict(hidden_sizes=())):
        with pytest.raises(NotImplementedError):
            AtariNoisyNetCatDqnPolicy(**_spec(**{k: v for k, v in kw.items() if k == "hidden_sizes"}),
                                      **{k: v for k, v in kw.items() if k != "hidden_sizes"})
    with pytest.raises(NotImplementedError):               # unchanged: the noisy Q-value policy has no dueling variant
        AtariNoisyNetDqnPolicy(dueling=True, **_spec())
    p = AtariNoisyNetCatDqnPolicy(n_atoms=2, dueling=True, common_noise=True, sigma_0=0.5, **_spec())
    assert p.get_epsilon() == 0
    p.set_epsilon(0.7)
    assert p.get_epsilon() == 0


def _noisy_ref(lrng, fan, units, norm, mu_init=True, sigma_0=0.4):
    wn = np.random.randn(fan, units).astype(np.float32)
    wn *= norm / np.sqrt(np.square(wn).sum(axis=0, keepdims=True))
    bb = np.zeros(units, np.float32)
    if mu_init:
        v = np.sqrt(1 / fan)
        wn = lrng.uniform(-v, v, (fan, units)).astype(np.float32)
        bb = lrng.uniform(-v, v, units).astype(np.float32)
    s = np.float32(sigma_0 / np.sqrt(fan))
    return [wn, bb, np.full((fan, units), s, np.float32), np.full(units, s, np.float32)]


@pytest.mark.parametrize("dueling", [False, True])
def test_names_shapes_init_order_and_round_trip(dueling):
    """Spec 0, 6 actions, 51 atoms: the reference's short names and shapes, its initial draws (noise seed first, conv
    Glorot weights, then per noisy layer in construction order NormCInit, uniform W, uniform b), a bit-exact round
    trip, and the stored layout's zero padding / off-block entries of W and W_sigma."""
    p = _host_policy(dueling)
    spec, n, a = _spec(), 51, 6
    np.random.seed(11)
    lrng = np.random.RandomState(11)
    noise_seed = np.random.randint(1, 123456)
    ref, c, h, w = [], 4, 104, 80
    for nf, sz, st, pad in zip(spec["conv_filters"], spec["conv_filter_sizes"], spec["conv_strides"], spec["conv_pads"]):
        fan_in, fan_out = c * sz * sz, nf * sz * sz
        lim = np.sqrt(6. / (fan_in + fan_out))
        ref += [lrng.uniform(-lim, lim, (nf, c, sz, sz)).astype(np.float32), np.zeros(nf, np.float32)]
        h, w, c = (h + 2 * pad[0] - sz) // st + 1, (w + 2 * pad[1] - sz) // st + 1, nf
    fan, hs = c * h * w, 256
    if dueling:
        hid, out = _noisy_ref(lrng, fan, hs, 1.0), _noisy_ref(lrng, hs, a * n, 0.01)
        hid_val, val = _noisy_ref(lrng, fan, hs, 1.0), _noisy_ref(lrng, hs, n, 0.01)
        ref += hid_val + val + hid + out
        names = ["FCVal0", "Val", "FC0", "Output"]
        shapes = [(fan, hs), (hs, n), (fan, hs), (hs, a * n)]
    else:
        ref += _noisy_ref(lrng, fan, hs, 1.0) + _noisy_ref(lrng, hs, a * n, 0.01)
        names, shapes = ["FC0", "Output"], [(fan, hs), (hs, a * n)]
    assert p.noise_seed == noise_seed and int(p._noise_state[0]) == noise_seed
    want_names = [nm + s for nm in names for s in ("W", "b", "Wsigma", "bsigma")]
    assert p.param_short_names[4:] == want_names
    assert [tuple(s) for s in p._ref_shapes[4:]] == [s for sh in shapes for s in (sh, sh[1:], sh, sh[1:])]
    flat = p.get_param_values()
    assert p.n_params == flat.size == sum(x.size for x in ref)
    np.testing.assert_array_equal(flat, np.concatenate([x.ravel() for x in ref]))
    scaled = flat * np.float32(1.5) + np.float32(0.25)
    p.set_param_values(scaled)
    np.testing.assert_array_equal(p.get_param_values(), scaled)
    s = p._atom_stride
    for k in (p._k_head, p._k_out_sigma):
        wk = p.params[k].detach().numpy().reshape(p._rows, s, -1)
        assert not wk[:, n:].any()                                         # atom padding
        if dueling:
            assert not wk[:a, :, hs:].any() and not wk[a, :, :hs].any()    # off-blocks
            assert wk[:a, :n, :hs].all() and wk[a, :n, hs:].all()


def test_rainbow_defaults_and_policy_checks():
    from accel_rl_amd.algos.dqn.rainbow import Rainbow
    from accel_rl_amd.policies.dqn.atari_cat_dqn_policy import AtariCatDqnPolicy
    from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy
    a = Rainbow()
    assert (a.reward_horizon, a.double_dqn, a.dueling_dqn, a.prioritized_replay, a.target_update_steps,
            a.min_steps_learn) == (3, True, True, True, 8000, 20000)
    o = a.optimizer
    assert (o._learning_rate, o._grad_norm_clip, o._scale_conv_grads, o._update_method.name) == (6.25e-5, 10, True, "adam")
    assert (a._eps_initial, a._eps_final, a._eps_eval) == (0, 0, 0)
    with pytest.raises(TypeError, match="AtariNoisyNetCatDqnPolicy"):
        a.build_loss(None, AtariCatDqnPolicy(dueling=True, **_spec()))
    with pytest.raises(ValueError, match="dueling"):
        a.build_loss(None, AtariNoisyNetCatDqnPolicy(dueling=False, **_spec()))
    with pytest.raises(ValueError, match="dueling"):
        Rainbow(dueling_dqn=False).build_loss(None, AtariNoisyNetCatDqnPolicy(dueling=True, **_spec()))


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def test_new_entry_points_reject_bad_arguments(lib):
    from accel_rl_amd import _lib
    buf = ctypes.c_void_p(16)           # never dereferenced: the argument checks come first
    # arl_noisy_draws
    assert lib.arl_noisy_draws(None, None, 1, 4, 1, None) == -1
    assert b"null" in lib.arl_last_error()
    draws = (_lib.ArlNoisyDraw * 2)()
    assert lib.arl_noisy_draws(buf, draws, 1, 4, 1, None) == -1                 # null f
    d = draws[0]
    d.f, d.width, d.pitch, d.layer, d.which = 16, 8, 8, 0, 0
    assert lib.arl_noisy_draws(buf, draws, 0, 4, 1, None) == -1                 # no draws
    assert lib.arl_noisy_draws(buf, draws, 1, 0, 1, None) == -1                 # no rows
    assert lib.arl_noisy_draws(buf, draws, 1, 4, 0, None) == -1                 # rows_per_draw
    assert lib.arl_noisy_draws(buf, draws, _lib.NOISY_MAX_DRAWS + 1, 4, 1, None) < 0
    d.which = 2
    assert lib.arl_noisy_draws(buf, draws, 1, 4, 1, None) == -1
    d.which, d.pitch = 0, 4                                                      # pitch < width
    assert lib.arl_noisy_draws(buf, draws, 1, 4, 1, None) == -1
    d.pitch, d.width = 8, 6                                                      # width % 4
    assert lib.arl_noisy_draws(buf, draws, 1, 4, 1, None) < 0
    d.width, d.which, d.x, d.xs = 8, 1, 16, 16                                   # x with an e_out draw
    assert lib.arl_noisy_draws(buf, draws, 1, 4, 1, None) == -1
    # arl_noisy_duel_combine
    item = _lib.ArlFoldItem()
    assert lib.arl_noisy_duel_combine(None, None, None, None, None, None, 4, 8, 4, 1, None, None, None, None, None) == -1
    item.part, item.total = 16, 32
    r = ctypes.byref(item)
    assert lib.arl_noisy_duel_combine(r, None, r, r, None, buf, 4, 8, 0, 1, buf, None, None, None, None) == -1  # split
    assert lib.arl_noisy_duel_combine(r, None, r, r, None, buf, 4, 8, 8, 1, buf, None, None, None, None) == -1
    assert lib.arl_noisy_duel_combine(r, None, r, r, None, buf, 4, 8, 4, 1, buf, buf, None, None, None) == -1  # xs_next
    item.splits = 2                                                              # total 32 != rows x split = 16
    assert lib.arl_noisy_duel_combine(r, None, r, r, None, buf, 4, 8, 4, 1, buf, None, None, None, None) == -1
    # arl_noisy_duel_bwd_prep / _bwd_dx
    assert lib.arl_noisy_duel_bwd_prep(None, None, 4, 8, 4, None, None, None, None, None) == -1
    assert lib.arl_noisy_duel_bwd_prep(buf, buf, 0, 8, 4, buf, buf, buf, buf, None) == -1
    assert lib.arl_noisy_duel_bwd_prep(buf, buf, 4, 8, 8, buf, buf, buf, buf, None) == -1
    assert lib.arl_noisy_duel_bwd_dx(None, None, None, None, None, 4, 8, None, None) == -1
    assert lib.arl_noisy_duel_bwd_dx(buf, buf, buf, buf, buf, 4, 0, buf, None) == -1
    assert lib.arl_noisy_duel_bwd_dx(buf, buf, buf, buf, buf, 4, 6, buf, None) < 0
    # the fused loss's limit query and launch
    assert lib.arl_noisy_catdqn_loss_limits(None, None, None) == -1
    max_splits, max_act, max_atoms = _lib.noisy_catdqn_loss_limits()
    assert max_splits == 128 and max_act == 64 and max_atoms == 64
    src = _lib.ArlNoisyLogitSrc()
    s = ctypes.byref(src)
    args = [buf] * 4 + [None, 4, 6, 51, 52, 0, -10., 10., 0.97, buf, buf, buf, None, 0, None]
    assert lib.arl_noisy_catdqn_loss_parts(None, None, None, *args) == -1
    assert lib.arl_noisy_catdqn_loss_parts(s, s, None, *args) == -1              # null pointers inside the source
    src.w_part, src.s_part, src.feout = 16, 16, 16
    bad = list(args)
    bad[7] = 65                                                                  # n_atoms
    assert lib.arl_noisy_catdqn_loss_parts(s, s, None, *bad) < 0
    bad = list(args)
    bad[10], bad[11] = 10., -10.                                                 # v_max <= v_min
    assert lib.arl_noisy_catdqn_loss_parts(s, s, None, *bad) == -1
    src.w_splits, src.w_split_stride = -1, 4
    assert lib.arl_noisy_catdqn_loss_parts(s, s, None, *args) == -1
    src.w_splits, src.s_splits, src.s_split_stride = max_splits, max_splits + 1, 4      # past the limit: ARL_E_RANGE
    rc = lib.arl_noisy_catdqn_loss_parts(s, s, None, *args)
    assert rc < 0 and rc != -1 and b"splits" in lib.arl_last_error()


@pytest.mark.parametrize("struct,macro", [("ArlNoisyDraw", ("ARL_NOISY_MAX_DRAWS", "NOISY_MAX_DRAWS")),
                                          ("ArlNoisyLogitSrc", ("ARL_NOISY_CATDQN_MAX_SPLITS", None))])
def test_new_structs_match_gcc(lib, struct, macro):
    from accel_rl_amd import _lib
    cls = getattr(_lib, struct)
    cname = {"ArlNoisyDraw": "arl_noisy_draw", "ArlNoisyLogitSrc": "arl_noisy_logit_src"}[struct]
    lines = ['printf("size %%zu\\n", sizeof(%s));' % cname, 'printf("max %%d\\n", %s);' % macro[0]]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], cname, f[0]) for f in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "accel_rl_hip.h"\nint main(){%s return 0;}' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "n.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "n")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    got = dict(zip(out[0::2], (int(v) for v in out[1::2])))
    assert got.pop("size") == ctypes.sizeof(cls)
    mx = got.pop("max")
    assert mx == (getattr(_lib, macro[1]) if macro[1] else _lib.noisy_catdqn_loss_limits()[0])
    for name, _ in cls._fields_:
        assert got[name] == getattr(cls, name).offset, name
