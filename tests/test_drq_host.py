"""DrQ without a device: the restatements of tests/drq_ref.py checked against what they must reproduce (Random123's
known answers, the uniformity of the offsets, float64), and the argument validation of DrQ, `augment_args` and
FrameReplayBuffer(augment=...), which is made before anything touches the device."""
import numpy as np
import pytest

import drq_ref as dr

GAMMA = float(np.float32(0.99 ** 3))


def test_philox_restatement_known_answers():
    """Random123's published Philox4x32-10 known-answer vectors (as tests/test_noisy_net_host.py)."""
    m = dr.MASK
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((m,) * 4, (m, m), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        assert [int(v) for v in dr.philox4x32_10(ctr, key)] == list(want)
    both = dr.philox4x32_10(([0, m], [0, m], [0, m], [0, m]), (0, 0))               # arrays broadcast
    assert [int(v) for v in both[0]] == list(cases[0][2])


def test_the_stream_constant_is_the_headers_and_apart_from_the_others():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "accel_rl_hip.h")).read()
    aug = int(re.search(r"#define ARL_AUG_PHILOX_STREAM (0x[0-9A-Fa-f]+)u", text).group(1), 16)
    iqn = int(re.search(r"#define ARL_IQN_PHILOX_STREAM (0x[0-9A-Fa-f]+)u", text).group(1), 16)
    assert aug == dr.AUG_STREAM and iqn == dr.IQN_STREAM and aug != iqn and 2 ** 31 <= aug < 2 ** 32


@pytest.mark.parametrize("pad", [0, 1, 4, 64])
def test_offsets_lie_inside_the_pad(pad):
    j, v = np.meshgrid(np.arange(500), np.arange(16), indexing="ij")
    for seed, call in ((0, 0), (-3, 2 ** 40 + 5), (2 ** 63 - 1, -1)):
        dx, dy = dr.shift_offsets(seed, call, j, v, pad)
        assert dx.shape == j.shape and dx.min() >= -pad and dx.max() <= pad and dy.min() >= -pad and dy.max() <= pad
        if pad:
            assert dx.min() == -pad and dx.max() == pad and dy.min() == -pad and dy.max() == pad
        else:
            assert not dx.any() and not dy.any()


def test_offsets_depend_on_every_counter_word_and_on_the_seed():
    j, v = np.meshgrid(np.arange(64), np.arange(4), indexing="ij")
    base = np.stack(dr.shift_offsets(7, 11, j, v, 4))
    for seed, call in ((8, 11), (7, 12), (7, 11 + 2 ** 32), (7 + 2 ** 32, 12)):
        assert not np.array_equal(np.stack(dr.shift_offsets(seed, call, j, v, 4)), base)
    assert np.array_equal(np.stack(dr.shift_offsets(7 + 2 ** 32, 11, j, v, 4)), base)     # the key holds (uint32) seed
    assert not np.array_equal(base[:, :, 0], base[:, :, 1]) and not np.array_equal(base[:, 0], base[:, 1])


def test_offsets_are_uniform_over_the_81_pairs():
    """81 x 2 000 draws at pad = 4 (seed 0; calls 0 .. 9, 1 000 samples, 8 + 8 views + 200 more): every pair occurs, and
    the chi-square statistic against the uniform law stays below the 99.9 % quantile of 80 degrees of freedom, 124.8."""
    n = 81 * 2000
    idx = np.arange(n)
    call, rest = idx // 16200, idx % 16200
    counts = np.zeros((9, 9), np.int64)
    for c in range(10):
        sel = rest[call == c]
        dx, dy = dr.shift_offsets(0, c, sel // 16, sel % 16, 4)
        np.add.at(counts, (dx + 4, dy + 4), 1)
    assert counts.sum() == n and counts.min() > 0
    chi2 = ((counts - 2000.) ** 2 / 2000.).sum()
    print("chi-square over the 81 offset pairs: %.1f (99.9 %% quantile of 80 d.o.f.: 124.8)" % chi2)
    assert chi2 < 124.8


def test_shifted_extract_is_a_pad_and_crop():
    """The restated gather against np.pad(mode="edge") + crop, blank frames zeroed first, on a toy ring."""
    rs = np.random.RandomState(1)
    n_env, size, f, h, w, hr = 2, 6, 3, 5, 8, 2
    store = dict(frames=rs.randint(0, 256, (n_env, size + f - 1, h * w), dtype=np.uint8),
                 n_blanks=rs.randint(0, f, (n_env, size + f - 1)).astype(np.uint8),
                 acts=rs.randint(0, 9, (n_env, size)).astype(np.uint8), returns=rs.randn(n_env, size).astype(np.float32),
                 terminals=rs.randint(0, 2, (n_env, size)).astype(np.uint8))
    env, step = [0, 1, 1], [0, 5, 3]
    obs, nxt, acts, rets, terms, offs = dr.shifted_extract(store, size, f, hr, h, w, env, step, 2, 2, 3, 5, 9)
    assert obs.shape == (6, f, h, w) and nxt.shape == (9, f, h, w) and len(set(map(tuple, offs.reshape(-1, 2)))) > 1
    for v in range(5):
        for j in range(3):
            i = (step[j] + hr) % size if v >= 2 else step[j]
            stack = store["frames"][env[j], i:i + f].reshape(f, h, w).copy()
            stack[:store["n_blanks"][env[j], i]] = 0
            dx, dy = offs[v, j]
            want = np.pad(stack, ((0, 0), (2, 2), (2, 2)), mode="edge")[:, 2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
            got = (nxt if v >= 2 else obs)[(v - 2 if v >= 2 else v) * 3 + j]
            assert np.array_equal(got, want)
    assert np.array_equal(acts, store["acts"][env, step]) and np.array_equal(rets, store["returns"][env, step])
    plain = dr.shifted_extract(store, size, f, hr, h, w, env, step, 0, 1, 1, 5, 9)
    assert not plain[5].any() and np.array_equal(plain[0][1], store["frames"][1, 5:5 + f].reshape(f, h, w) *
                                                 (np.arange(f) >= store["n_blanks"][1, 5])[:, None, None])


LOSS_GRID = [(a, b, duel, dbl, wtd, clip) for (a, b) in ((4, 1), (18, 37), (64, 5)) for duel in (False, True)
             for dbl in (False, True) for wtd in (False, True) for clip in (1.0, 0.25, 0.0)]


def _seed(a, b, duel, dbl, wtd, clip, k, m):
    return 1000 * a + 10 * b + 4 * duel + 2 * dbl + wtd + int(100 * clip) + 7 * k + 13 * m


@pytest.mark.parametrize("k,m", [(1, 1), (2, 2), (1, 3), (8, 8)])
def test_fp32_emulation_agrees_with_float64_within_the_derived_bound(k, m):
    worst, kept, total = 0., 0, 0
    for a, b, duel, dbl, wtd, clip in LOSS_GRID:
        c = dr.drq_case(_seed(a, b, duel, dbl, wtd, clip, k, m), a, b, k, m, duel, dbl, wtd)
        dq, rows, td = dr.emu_drq32(c, GAMMA, clip)
        ref = dr.ref_drq64(c, GAMMA, clip)
        ok = ref["ok"]
        kept, total = kept + ok.sum(), total + b
        okv = np.tile(ok, m)
        cols = a + int(duel)
        assert not dq[:, cols:].any()
        errs = [(np.abs(dq[:, :cols] - ref["dq"]).max(axis=1)[okv], ref["dq_tol"][okv]),
                (np.abs(rows - ref["rows"])[ok], ref["rows_tol"][ok]), (np.abs(td - ref["td"])[ok], ref["td_tol"][ok])]
        for err, tol in errs:
            assert (err <= tol).all(), (a, b, duel, dbl, wtd, clip, (err / tol).max())
            worst = max(worst, (err / np.maximum(tol, 1e-300)).max())
    print("k %d m %d: largest error / bound %.3f; the reference keeps %d of %d samples" % (k, m, worst, kept, total))
    assert kept >= 0.95 * total


def test_k_m_1_is_the_dqn_loss_bit_for_bit():
    for a, b, duel, dbl, wtd, clip in LOSS_GRID:
        c = dr.drq_case(_seed(a, b, duel, dbl, wtd, clip, 1, 1), a, b, 1, 1, duel, dbl, wtd, delta_clip=clip, special=True)
        for x, y in zip(dr.emu_drq32(c, GAMMA, clip), dr.emu_dqn32(c, GAMMA, clip)):
            assert x.dtype == np.float32 and np.array_equal(x, y)


def test_special_rows_are_what_they_claim():
    c = dr.drq_case(5, 18, 37, 2, 3, True, True, True, delta_clip=0.25, special=True)
    _, _, td = dr.emu_drq32(c, GAMMA, 0.25)
    assert (td[0::5] == np.float32(0.25)).all()                 # |d_v| == delta_clip exactly, in every view
    for key in ("nxt", "pol"):
        tied = c[key].reshape(2, 37, -1)[:, 1::5, :18]
        assert ((tied == tied.max(axis=2, keepdims=True)).sum(axis=2) == 2).all()
    # the first of two equal maxima is taken
    d = dr.drq_case(5, 18, 37, 2, 3, False, False, False, special=True)
    row = d["nxt"][1]
    at = np.flatnonzero(row[:18] == row[:18].max())
    assert len(at) == 2 and np.argmax(row[:18]) == at[0] and dr._next32(d, 0)[1] == row[at[0]]


# ---- argument validation (no device) ---------------------------------------------------------------------------------

def test_drq_defaults_and_refusals():
    from accel_rl_amd.algos.dqn.drq import DrQ
    from accel_rl_amd.optimizers import update_methods
    algo = DrQ()
    assert (algo.double_dqn, algo.dueling_dqn, algo.reward_horizon, algo.batch_size) == (True, True, 10, 32)
    assert (algo.replay_size, algo.min_steps_learn, algo.training_intensity, algo.target_update_steps) == (100000, 1600, 32, 1)
    assert (algo._eps_initial, algo._eps_final, algo._eps_eval, algo._eps_anneal_steps) == (1., 0.1, 0.05, 5000)
    opt = algo.optimizer
    assert opt._learning_rate == 1e-4 and opt._update_method is update_methods.adam and opt._grad_norm_clip == 10
    assert algo._replay_augment == dict(pad=4, seed=0, m_obs=1, k_next=1)
    assert DrQ(k_targets=2, m_online=3, pad=2, aug_seed=9)._replay_augment == dict(pad=2, seed=9, m_obs=3, k_next=2)
    assert DrQ(prioritized_replay=True).prioritized_replay and not DrQ(double_dqn=False).double_dqn
    for kw in (dict(k_targets=0), dict(k_targets=9), dict(m_online=0), dict(m_online=9), dict(m_online=1.5), dict(pad=-1),
               dict(pad=65)):
        with pytest.raises(ValueError):
            DrQ(**kw)
    with pytest.raises(TypeError, match="augment_args"):
        DrQ(augment_args=dict(pad=4))

    class Sub(__import__("accel_rl_amd.policies.dqn.atari_dqn_policy", fromlist=["x"]).AtariDqnPolicy):
        pass
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    with pytest.raises(TypeError, match="AtariDqnPolicy itself"):
        algo.build_loss(None, Sub(dueling=True, **dict(cnn_specs[0], hidden_sizes=[64])))
    with pytest.raises(TypeError, match="AtariDqnPolicy itself"):
        algo.build_loss(None, object())


def test_augment_args_of_the_family():
    from accel_rl_amd.algos.dqn.cat_dqn import CategoricalDQN
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.algos.dqn.fqf import FQF
    from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
    from accel_rl_amd.algos.dqn.munchausen import MunchausenDQN, MunchausenIQN
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.algos.dqn.rainbow import Rainbow
    for cls in (DQN, CategoricalDQN, Rainbow, QuantileDQN, ImplicitQuantileDQN, MunchausenDQN, MunchausenIQN, FQF):
        assert cls()._replay_augment is None
        assert cls(augment_args=dict())._replay_augment == dict(pad=4, seed=0, m_obs=1, k_next=1)
        assert cls(augment_args=dict(pad=2, seed=5))._replay_augment == dict(pad=2, seed=5, m_obs=1, k_next=1)
        for bad in (dict(k_targets=2), dict(m_online=2)):
            with pytest.raises(NotImplementedError, match="DrQ"):
                cls(augment_args=bad)
        with pytest.raises(TypeError, match="intensity"):
            cls(augment_args=dict(intensity=0.05))
        with pytest.raises(ValueError):
            cls(augment_args=dict(pad=65))


def test_replay_buffer_augment_is_checked_before_the_device():
    from accel_rl_amd.algos.dqn.replay_buffers.frame import FrameReplayBuffer
    check = FrameReplayBuffer._check_augment
    assert check(None, (104, 80)) is None
    assert check(dict(), (104, 80)) == dict(pad=4, seed=0, m_obs=1, k_next=1, call=0)
    assert check(dict(pad=0, seed=3, m_obs=8, k_next=2), (4, 4)) == dict(pad=0, seed=3, m_obs=8, k_next=2, call=0)
    for shape in ((104, 82), (8320,), (2, 52, 80), ()):
        with pytest.raises(NotImplementedError, match="multiple of 4"):
            check(dict(), shape)
    for bad in (dict(pad=-1), dict(pad=65), dict(m_obs=0), dict(m_obs=9), dict(k_next=0), dict(k_next=9)):
        with pytest.raises(ValueError):
            check(bad, (104, 80))
    with pytest.raises(TypeError):
        check(dict(pad=1.5), (104, 80))
    with pytest.raises(TypeError, match="unexpected"):
        check(dict(shift=4), (104, 80))

    class Space(object):
        shape = (4, 104, 82)

    class Spec(object):
        observation_space = Space()
    with pytest.raises(NotImplementedError, match="multiple of 4"):      # at construction, before any allocation
        FrameReplayBuffer(Spec(), 64, 1, 4, 2, 0.99, device="cpu", augment=dict(pad=4))


def test_the_new_entry_points_are_exported_and_refuse_without_a_device():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    for name in ("arl_replay_extract_shift", "arl_drq_loss"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.arl_drq_loss(None, None, None, None, None, None, None, 4, 1, 1, 4, 4, 0, 0.99, 1.0, None, None, None, None) == -1
    assert b"null" in lib.arl_last_error()
    assert lib.arl_replay_extract_shift(None, None, None, 4, 4, 4, 4, 1, 1, 0, 0, None, None, None, None, None, None) == -1
    assert callable(_lib.replay_extract_shift) and callable(_lib.drq_loss)
