"""CPU-only checks of the noisy-net layer's C-ABI (csrc/noisy.hip, include/accel_rl_hip.h): argument errors without a
GPU, the arl_noisy_layer mirror's layout against gcc, and the numpy restatement of the generator the GPU tests compare
the device against (Philox4x32-10 known-answer vectors, Box-Muller, f)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 on arrays: ctr uint64[..., 4] (values < 2^32), key (k0, k1) arrays -> uint64[..., 4] words."""
    c = [np.asarray(ctr[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[0], np.uint64), np.asarray(key[1], np.uint64)
    for i in range(10):
        if i > 0:
            k0, k1 = (k0 + np.uint64(_W0)) & np.uint64(_MASK), (k1 + np.uint64(_W1)) & np.uint64(_MASK)
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, axis=-1)


def noisy_words_normals(seed, counter, layer, which, rows, width, rows_per_draw=1):
    """The header's generator: (words uint32[rows][width], e float32[rows][width], f(e) float32[rows][width])."""
    j = np.arange(width)
    r = np.arange(rows)
    q = (j // 4)[None, :].repeat(rows, 0)
    g = (r // rows_per_draw)[:, None].repeat(width, 1)
    ctr = np.stack([q, g, np.full_like(q, counter & _MASK), np.full_like(q, (counter >> 32) & _MASK)], axis=-1)
    w = philox4x32_10(ctr.astype(np.uint64), (np.uint64(seed & _MASK), np.uint64(2 * layer + which)))
    lane = (j % 4)[None, :]
    pair = lane // 2
    w_u1 = np.take_along_axis(w, (2 * pair)[..., None].repeat(rows, 0), axis=-1)[..., 0]
    w_u2 = np.take_along_axis(w, (2 * pair + 1)[..., None].repeat(rows, 0), axis=-1)[..., 0]
    u1 = ((w_u1 >> np.uint64(8)).astype(np.float64) + 0.5) / 2.0 ** 24
    u2 = ((w_u2 >> np.uint64(8)).astype(np.float64) + 0.5) / 2.0 ** 24
    rad = np.sqrt(-2.0 * np.log(u1))
    e = np.where(lane % 2 == 0, rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)).astype(np.float32)
    words = np.take_along_axis(w, lane[..., None].repeat(rows, 0), axis=-1)[..., 0].astype(np.uint32)
    f = (np.sign(e) * np.sqrt(np.abs(e))).astype(np.float32)
    return words, e, f


def test_philox_restatement_known_answers():
    """Random123's published Philox4x32-10 known-answer vectors."""
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((_MASK,) * 4, (_MASK, _MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = philox4x32_10(np.array([ctr], np.uint64), (np.uint64(key[0]), np.uint64(key[1])))[0]
        assert [int(v) for v in got] == list(want)


def test_generator_restatement_shapes_and_groups():
    words, e, f = noisy_words_normals(7, 3, 1, 0, 6, 10, rows_per_draw=3)
    assert words.shape == e.shape == f.shape == (6, 10)
    np.testing.assert_array_equal(e[0], e[2])
    assert not np.array_equal(e[0], e[3])
    np.testing.assert_array_equal(np.sign(f), np.sign(e))
    np.testing.assert_allclose(f * f, np.abs(e), rtol=1e-6)
    assert not np.array_equal(noisy_words_normals(7, 4, 1, 0, 1, 8)[1], noisy_words_normals(7, 3, 1, 0, 1, 8)[1])
    assert not np.array_equal(noisy_words_normals(7, 3, 1, 1, 1, 8)[1], noisy_words_normals(7, 3, 1, 0, 1, 8)[1])


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def test_noisy_entry_points_reject_bad_arguments(lib):
    from accel_rl_amd import _lib
    assert lib.arl_noisy_normals(1, 0, 0, 0, 4, 8, 1, None, None, None, None) == -1
    assert b"null" in lib.arl_last_error()
    buf = ctypes.c_void_p(16)           # never dereferenced: the size checks come first
    assert lib.arl_noisy_normals(1, 0, 0, 2, 4, 8, 1, buf, None, None, None) == -1
    assert lib.arl_noisy_normals(1, 0, 0, 0, 0, 8, 1, buf, None, None, None) == -1
    assert lib.arl_noisy_normals(1, 0, 0, 0, 4, 8, 0, buf, None, None, None) == -1
    assert lib.arl_noisy_noise(None, None, 1, 4, 1, None) == -1
    layers = (_lib.ArlNoisyLayer * 1)()
    assert lib.arl_noisy_noise(buf, layers, 1, 4, 1, None) == -1          # null buffers inside the layer
    assert b"null" in lib.arl_last_error()
    assert lib.arl_noisy_noise(buf, layers, 0, 4, 1, None) == -1
    item = _lib.ArlFoldItem()
    assert lib.arl_noisy_dense_combine(None, None, None, None, None, 4, 8, 1, None, None, None, None, None) == -1
    assert lib.arl_noisy_dense_combine(ctypes.byref(item), None, ctypes.byref(item), None, buf, 4, 8, 1, buf, None,
                                       None, None, None) == -1           # item.part null
    assert lib.arl_noisy_dense_bwd_prep(None, None, 4, 8, None, None, None, None) == -1
    assert lib.arl_noisy_dense_bwd_prep(buf, buf, 0, 8, buf, buf, buf, None) == -1
    assert lib.arl_noisy_dense_bwd_dx(None, None, None, 4, 8, None, None) == -1
    assert lib.arl_noisy_dense_bwd_dx(buf, buf, buf, 4, 0, buf, None) == -1
    assert lib.arl_last_error()


def test_noisy_layer_struct_matches_gcc(lib):
    from accel_rl_amd import _lib
    lines = ['printf("size %zu\\n", sizeof(arl_noisy_layer));', 'printf("max %d\\n", ARL_NOISY_MAX_LAYERS);']
    lines += ['printf("%s %%zu\\n", offsetof(arl_noisy_layer, %s));' % (f[0], f[0]) for f in _lib.ArlNoisyLayer._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "accel_rl_hip.h"\nint main(){%s return 0;}' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "n.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "n")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    got = dict(zip(out[0::2], (int(v) for v in out[1::2])))
    assert got.pop("size") == ctypes.sizeof(_lib.ArlNoisyLayer)
    assert got.pop("max") == _lib.NOISY_MAX_LAYERS
    for name, _ in _lib.ArlNoisyLayer._fields_:
        assert got[name] == getattr(_lib.ArlNoisyLayer, name).offset, name


def test_non_factorized_and_dueling_are_refused():
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    with pytest.raises(NotImplementedError):
        AtariNoisyNetDqnPolicy(factorized=False, **cnn_specs[0])
    with pytest.raises(NotImplementedError):
        AtariNoisyNetDqnPolicy(dueling=True, **cnn_specs[0])
    p = AtariNoisyNetDqnPolicy(common_noise=True, sigma_0=0.5, **cnn_specs[0])
    assert p.get_epsilon() == 0
    p.set_epsilon(0.7)
    assert p.get_epsilon() == 0
