"""Rectifier masks as bits (y_bits_or_null / mask_bits_or_null of the arl_conv2d_* calls, AtariCnnPolicy._relu_bits_layers, ARL_RELU_BITS): the forward kernels of the
learner's conv layers also write `y > 0` as one bit per value, u32[rows][C / 32], and the data gradients read those
words instead of the f32 activations.  Nothing is computed differently -- only where a comparison's outcome is read from
changes -- so everything here is exact: the words against numpy's packing of the same launch's f32 output, dx with bits
against dx with the f32 mask (torch.equal), whole PPO updates with the switch on and off, and the refusals.

Shapes (spec 1's layers at the smallest sizes that reach every branch): batch 3 gives conv 2 / conv 3 324 rows -- two full
128-row tiles and a ragged one -- and the stride-2 data gradient four parity classes of 3 x (13 x 10, 13 x 9, 12 x 10,
12 x 9) = 390, 351, 360, 324 pixels, the last row tile of each ragged; conv 1 has 475 pixels per image (14 full 32-pixel
tiles and one of 27).  The dense layer's data gradient at 130 rows is below the size at which it shares a launch with
the weight gradient (130 x 6912 <= 2^20 elements: its reduction is split and the fold compares the f32 mask, bits or
not); 160 rows is the smallest multiple of 32 above that size and runs the shared launch, which reads the bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 64, 0x5A5A5A5A

CONV1 = dict(in_h=104, in_w=80, in_c=4, out_c=32, k=8, stride=4, pad=0)     # -> 25 x 19 x 32
CONV2 = dict(in_h=25, in_w=19, in_c=32, out_c=64, k=4, stride=2, pad=1)     # -> 12 x 9 x 64
CONV3 = dict(in_h=12, in_w=9, in_c=64, out_c=64, k=3, stride=1, pad=1)      # -> 12 x 9 x 64


def pack_bits(y, channels):
    """u32[rows][channels / 32] of (y > 0), bit c % 32 of word c // 32 -- numpy alone."""
    m = (np.asarray(y, np.float32).reshape(-1, channels) > 0)
    return np.packbits(m, axis=-1, bitorder="little").view("<u4").reshape(-1, channels // 32)


def crafted(rows, channels, seed):
    """A mask tensor f32[rows][channels] with about half zeros, among them -0.0, negatives and a NaN; row 0 all zeros,
    row 1 none; row 2's first word has bit 0 alone, row 3's last word bit 31 alone."""
    rng = np.random.RandomState(seed)
    y = rng.standard_normal((rows, channels)).astype(np.float32)
    y[y < 0] = 0.0
    y[rng.rand(rows, channels) < 0.05] = -0.0
    y[rng.rand(rows, channels) < 0.02] = -1.5
    y[4, 3] = np.nan
    y[0, :] = 0.0
    y[1, :] = np.abs(rng.standard_normal(channels).astype(np.float32)) + 0.5
    y[2, :32] = 0.0
    y[2, 0] = 2.0
    y[3, -32:] = -0.0
    y[3, -1] = 1e-30
    return y


def test_crafted_masks_hold_the_edge_words():
    """(CPU) the handcrafted masks of the consumer cases contain what they are meant to, by numpy's packing alone."""
    for rows, ch in ((3 * 25 * 19, 32), (3 * 12 * 9, 64), (130, 6912)):
        y = crafted(rows, ch, 1)
        w = pack_bits(y, ch)
        assert w.dtype == np.uint32 and w.shape == (rows, ch // 32)
        assert not w[0].any() and (w[1] == 0xFFFFFFFF).all()
        assert w[2, 0] == 1 and w[3, -1] == 0x80000000
        assert 0.3 < (y > 0).mean() < 0.6 and np.signbit(y[y == 0]).any() and np.isnan(y).any()
        assert not (w[4, 0] >> 3) & 1                       # the NaN is not > 0
    one = np.zeros((1, 64), np.float32)
    one[0, 33] = 1.0
    assert pack_bits(one, 64).tolist() == [[0, 2]]


# ---- helpers (GPU)

def geom_of(layer, batch):
    from accel_rl_amd import _lib
    return _lib.conv_geom(batch, layer["in_h"], layer["in_w"], layer["in_c"], layer["out_c"], layer["k"], layer["k"],
                          layer["stride"], layer["pad"], layer["pad"])


def out_hw(layer):
    return ((layer["in_h"] + 2 * layer["pad"] - layer["k"]) // layer["stride"] + 1,
            (layer["in_w"] + 2 * layer["pad"] - layer["k"]) // layer["stride"] + 1)


def randn(shape, seed, scale=1.0):
    return (torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed)) * scale).contiguous()


def guarded(n_words):
    """(whole buffer, the n_words in its middle): guard words on both sides, everything at the fill value."""
    buf = torch.full((n_words + 2 * GUARD,), FILL, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + n_words]


def check_words(buf, bits, y, channels):
    torch.cuda.synchronize()
    got = bits.cpu().numpy().view(np.uint32).reshape(-1, channels // 32)
    want = pack_bits(y.cpu().numpy(), channels)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert 0.2 < (y > 0).float().mean().item() < 0.8        # a real mixture, not all or nothing
    g = buf.cpu().numpy()
    assert (g[:GUARD] == FILL).all() and (g[-GUARD:] == FILL).all()


class fwd_tile(object):
    """The 33 .. 64-column kernels' tile under arl_dev_fwd_tile: 0 = 128 x 64 (TN = 2: the shape the learner's 512-row
    minibatch takes by its size), -1 = by size (three row tiles: two 32-column tiles per row tile)."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from accel_rl_amd import _lib
        _lib.load().arl_dev_fwd_tile(self.v)

    def __exit__(self, *exc):
        from accel_rl_amd import _lib
        _lib.load().arl_dev_fwd_tile(-1)


_ws = {}


def workspace():
    from accel_rl_amd import _lib
    if "ws" not in _ws:
        _ws["ws"] = _lib.conv_workspace(DEV)
    return _ws["ws"]


# ---- producers

@gpu
@pytest.mark.parametrize("tile", [0, -1], ids=["tn2", "by_size"])
@pytest.mark.parametrize("layer", [CONV2, CONV3], ids=["conv2", "conv3"])
def test_forward_writes_the_bits_of_its_own_output(layer, tile):
    with fwd_tile(tile):
        _forward_case(layer, (4, 1, 1, 2) if tile == 0 else (4, 1, 1, 1))


def _forward_case(layer, shape):
    from accel_rl_amd import _lib
    b = 3
    g = geom_of(layer, b)
    ho, wo = out_hw(layer)
    rows, ch = b * ho * wo, layer["out_c"]
    assert rows == 324
    x = randn((b, layer["in_h"], layer["in_w"], layer["in_c"]), 1).abs_()
    w = randn((ch, layer["k"], layer["k"], layer["in_c"]), 2, 0.05)
    bias = randn((ch,), 3, 0.1)
    y0 = torch.full((rows, ch), -7.0, device=DEV)
    y1 = torch.full((rows, ch), -7.0, device=DEV)
    _lib.conv2d_fwd(x, w, bias, y0, g, True, workspace())
    plain = _lib.conv_launch_log()
    buf, bits = guarded(rows * ch // 32)
    _lib.conv2d_fwd(x, w, bias, y1, g, True, workspace(), y_bits=bits.view(_lib.relu_bits_shape(rows, ch)))
    with_bits = _lib.conv_launch_log()
    assert [(r.family, r.tile, r.grid) for r in plain] == [(r.family, r.tile, r.grid) for r in with_bits]
    assert [(r.family, r.tile[:4]) for r in plain] == [("igemm_split", shape)]
    check_words(buf, bits, y1, ch)
    assert torch.equal(y0, y1)
    # without the rectifier the bits are still those of the stored values
    y2 = torch.empty_like(y1)
    buf, bits = guarded(rows * ch // 32)
    _lib.conv2d_fwd(x, w, bias, y2, g, False, workspace(), y_bits=bits.view(rows, ch // 32))
    check_words(buf, bits, y2, ch)
    assert (y2 < 0).any()


@gpu
@pytest.mark.parametrize("route", ["split9", "bf16"])
@pytest.mark.parametrize("batch,indexed", [(1, False), (3, True)], ids=["b1", "b3_idx"])
def test_conv1_from_u8_writes_the_bits_of_its_own_output(batch, indexed, route):
    """route bf16: the image-stationary kernel does not take the one-product route; the tap-gathering split kernel
    (128-row tiles, two row tiles per wave) runs in its place and writes the bits as well."""
    from accel_rl_amd import _lib
    g = geom_of(CONV1, batch)
    g.route = _lib.ROUTE_SPLIT9 if route == "split9" else _lib.ROUTE_BF16
    family = "conv1_img" if route == "split9" else "igemm_split"
    ho, wo = out_hw(CONV1)
    rows, ch = batch * ho * wo, 32
    n_obs = 5 if indexed else batch
    obs = torch.randint(0, 256, (n_obs, 4, 104, 80), device=DEV, generator=torch.Generator(DEV).manual_seed(4)).to(torch.uint8)
    idx = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV) if indexed else None
    w = randn((32, 4, 8, 8), 5, 0.05)
    bias = randn((32,), 6, 0.3)
    y0 = torch.full((rows, ch), -7.0, device=DEV)
    y1 = torch.full((rows, ch), -7.0, device=DEV)
    _lib.conv2d_u8_fwd(obs, idx, 1.0 / 255, w, bias, y0, g, True)
    assert [r.family for r in _lib.conv_launch_log()] == [family]
    buf, bits = guarded(rows)
    _lib.conv2d_u8_fwd(obs, idx, 1.0 / 255, w, bias, y1, g, True, y_bits=bits.view(rows, 1))
    assert [r.family for r in _lib.conv_launch_log()] == [family]
    check_words(buf, bits, y1, ch)
    assert torch.equal(y0, y1)


# ---- consumers

def masks_for(layer_below, b, producer_seed):
    """[(name, mask f32 [rows][C], bits i32 [rows][C / 32])]: a handcrafted mask with numpy's packing, and a real forward's
    output with the bits that forward wrote."""
    from accel_rl_amd import _lib
    ho, wo = out_hw(layer_below)
    rows, ch = b * ho * wo, layer_below["out_c"]
    y = crafted(rows, ch, producer_seed)
    out = [("crafted", torch.from_numpy(y).to(DEV), torch.from_numpy(pack_bits(y, ch).view(np.int32)).to(DEV))]
    yp = torch.empty((rows, ch), device=DEV)
    bits = torch.zeros(_lib.relu_bits_shape(rows, ch), dtype=torch.int32, device=DEV)
    if layer_below is CONV1:
        obs = torch.randint(0, 256, (b, 4, 104, 80), device=DEV, generator=torch.Generator(DEV).manual_seed(7)).to(torch.uint8)
        _lib.conv2d_u8_fwd(obs, None, 1.0 / 255, randn((32, 4, 8, 8), 8, 0.05), randn((32,), 9, 0.3), yp, geom_of(CONV1, b),
                           True, y_bits=bits)
    else:
        x = randn((b, layer_below["in_h"], layer_below["in_w"], layer_below["in_c"]), 7).abs_()
        w = randn((ch, layer_below["k"], layer_below["k"], layer_below["in_c"]), 8, 0.05)
        _lib.conv2d_fwd(x, w, randn((ch,), 9, 0.1), yp, geom_of(layer_below, b), True, workspace(), y_bits=bits)
    out.append(("produced", yp, bits))
    return out


@gpu
@pytest.mark.parametrize("layer,below,tile", [(CONV2, CONV1, -1), (CONV3, CONV2, 0), (CONV3, CONV2, -1)],
                         ids=["conv2", "conv3_tn2", "conv3_by_size"])
def test_data_gradient_with_bits_is_the_data_gradient(layer, below, tile):
    """conv 2's data gradient (stride 2: four parity classes of unequal size, <4,1,1,1> tiles) and conv 3's (TN = 2, the
    bits prefetched; and the two-column-tile launch its three row tiles take by size): dx with the bits == dx with the f32
    mask, with and without the k-contiguous weight copy (without it the launch has no bit path and compares the floats:
    still the same dx)."""
    with fwd_tile(tile):
        _dgrad_case(layer, below, (4, 1, 1, 2) if tile == 0 else (4, 1, 1, 1))


def _dgrad_case(layer, below, shape):
    from accel_rl_amd import _lib
    b = 3
    g = geom_of(layer, b)
    ho, wo = out_hw(layer)
    dy = randn((b, ho, wo, layer["out_c"]), 11)
    w = randn((layer["out_c"], layer["k"], layer["k"], layer["in_c"]), 12, 0.05)
    wt = torch.empty_like(w)
    _lib.conv2d_dgrad_weights([(w.view(-1), wt.view(-1), g)])
    for name, mask, bits in masks_for(below, b, 13):
        for use_wt in (wt, None):
            dx0 = torch.full_like(mask, 9.0)
            dx1 = torch.full_like(mask, 9.0)
            _lib.conv2d_bwd_data(dy, w, mask, dx0, g, wt=use_wt)
            plain = [(r.family, r.tile, r.grid) for r in _lib.conv_launch_log()]
            _lib.conv2d_bwd_data(dy, w, mask, dx1, g, wt=use_wt, mask_bits=bits)
            assert plain == [(r.family, r.tile, r.grid) for r in _lib.conv_launch_log()]
            assert plain[0][0] == "igemm_split" and plain[0][1][:4] == shape
            torch.cuda.synchronize()
            assert torch.equal(dx0, dx1), (name, use_wt is not None)
            keep = mask > 0
            assert bool((dx0[~keep] == 0).all()) and float(dx0[keep].abs().sum()) > 0
        # wrong bits give another dx: the launch with the weight copy does read them
        dx2 = torch.full_like(mask, 9.0)
        _lib.conv2d_bwd_data(dy, w, mask, dx2, g, wt=wt, mask_bits=torch.zeros_like(bits))
        torch.cuda.synchronize()
        assert float(dx2.abs().sum()) == 0.0, name


@gpu
@pytest.mark.parametrize("rows,shared", [(130, False), (160, True)], ids=["130", "160"])
def test_dense_pair_with_bits_is_the_dense_pair(rows, shared):
    """The dense layer (6912 -> 512) through FoldList.conv2d_bwd_pair.  130 rows: below the shared launch's size, the data
    gradient splits its reduction and the fold compares the f32 mask whatever the bits say.  160 rows: the shared launch
    (bwd_pair), whose data-gradient tiles read the bits."""
    from accel_rl_amd import _lib
    fan_in, units = 6912, 512
    g = _lib.dense_geom(rows, fan_in, units)
    dy = randn((rows, units), 21)
    w = randn((units, fan_in), 22, 0.02)
    y = crafted(rows, fan_in, 23)
    mask = torch.from_numpy(y).to(DEV)
    mask[4, 3] = 0.0                    # (the mask is also the layer's input x: keep the weight gradient finite)
    bits = torch.from_numpy(pack_bits(mask.cpu().numpy(), fan_in).view(np.int32)).to(DEV)
    outs = []
    for mb in (None, bits, torch.zeros_like(bits)):
        folds = _lib.FoldList()
        dx = torch.full((rows, fan_in), 9.0, device=DEV)
        dw = torch.zeros((units, fan_in), device=DEV)
        db = torch.zeros(units, device=DEV)
        ws = _lib.conv_workspace(DEV)
        # (130 rows: no multiple of the weight gradient's 32-row k-tile -- the generic kernels, which leave no bias sums)
        assert folds.conv2d_bwd_pair(dy, w.view(-1), mask, dx, mask, dw.view(-1), g, ws, dbias=db, mask_bits=mb) == shared
        fams = [r.family for r in _lib.conv_launch_log()]
        folds.run()
        torch.cuda.synchronize()
        outs.append((dx, dw, db, fams))
    assert outs[0][3] == outs[1][3] and ("bwd_pair" in outs[0][3]) == shared, outs[0][3]
    for a, c in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, c)
    keep = mask > 0
    assert bool((outs[0][0][~keep] == 0).all()) and float(outs[0][0][keep].abs().sum()) > 0
    # all-zero bits: the shared launch reads them (dx = 0); the split reduction's fold never does
    assert (float(outs[2][0].abs().sum()) == 0.0) == shared
    assert torch.equal(outs[2][1], outs[0][1]) and torch.equal(outs[2][2], outs[0][2])


# ---- the policy's plumbing: whole PPO updates with the switch on and off

def build_ppo(use_graph, seed=5):
    from accel_rl_amd.algos.pg.ppo import PPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="breakout"), horizon=5, n_parallel=2, envs_per=2,
                            max_path_length=int(27e3), mid_batch_reset=True, max_decorrelation_steps=0, device=DEV,
                            use_graph=use_graph)
    algo = PPO(discount=0.99, gae_lambda=0.95, optimizer_args=dict(minibatch_size=16, epochs=2), use_graph=use_graph)
    policy = AtariCnnPolicy(**cnn_specs[1])
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=seed, log_interval_steps=1e8)
    runner.startup()
    with torch.no_grad():       # sharpen the heads and move every bias off zero (a fresh network's masks are lopsided)
        policy.flat_params[policy._offsets[policy._k_head]:].mul_(40.0)
        for k in range(1, 2 * (policy._n_conv + policy._n_hid), 2):
            policy._w[k].add_(0.01 * torch.randn(policy._w[k].shape, device=DEV,
                                                 generator=torch.Generator(DEV).manual_seed(k)))
    return runner, sampler, algo, policy


@gpu
@pytest.mark.parametrize("first_reused", [False, True], ids=["all_computed", "first_reused"])
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_ppo_updates_are_the_same_with_and_without_bits(captured, first_reused, monkeypatch):
    """PPO, 8 envs x horizon 5, minibatches of 16 rows x 2 epochs, the rollout's store offered: two optimize_policy calls
    (captured: after one eager warm-up call, the two from the learner's hipGraph) with ARL_RELU_BITS at its default and
    two with ARL_RELU_BITS=0 from the same seed -- parameters, both optimiser slots, the step count, every minibatch's
    loss4 (eager) and the returned gradient norms bit for bit.  first_reused: the call's first minibatch takes the
    rollout's activations (no producer ran for it: it keeps the f32 masks); otherwise ARL_REUSE_ACTS=0 and every
    minibatch's forward writes its bits."""
    from accel_rl_amd import _lib
    monkeypatch.setenv("ARL_REUSE_ACTS", "1" if first_reused else "0")
    outs, used = [], []
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("ARL_RELU_BITS", raising=False)
        else:
            monkeypatch.setenv("ARL_RELU_BITS", switch)
        n_bits = [0]
        real = _lib.FoldList.conv2d_bwd_pair

        def spy(self, *args, **kwargs):
            n_bits[0] += kwargs.get("mask_bits") is not None
            return real(self, *args, **kwargs)
        monkeypatch.setattr(_lib.FoldList, "conv2d_bwd_pair", spy)
        runner, sampler, algo, policy = build_ppo(captured)
        assert policy._relu_bits_layers() == ((0, 1, 2) if switch is None else ())
        np.random.seed(31)
        losses, norms = [], []
        inner = algo.optimizer._losses

        def recorded(mb):
            loss4 = inner(mb)
            if not torch.cuda.is_current_stream_capturing():
                losses.append(loss4.clone())
            return loss4
        algo.optimizer._losses = recorded
        for itr in range(3 if captured else 2):
            samples, _ = sampler.obtain_samples(itr)
            assert algo._reuse_granted(samples) == first_reused
            if captured and itr == 1:
                algo._warm_calls = 2                # (the second call captures both flavours and replays)
            _, infos = algo.optimize_policy(itr, samples)
            norms.append(infos["GradNorm"].clone())
        torch.cuda.synchronize()
        assert bool(algo._graphs) == captured
        opt = algo.optimizer
        outs.append([policy.flat_params.clone(), opt._slot0.clone(), opt._slot1.clone(), opt._step_count.clone()] +
                    losses + norms)
        used.append(n_bits[0])
        monkeypatch.setattr(_lib.FoldList, "conv2d_bwd_pair", real)
        algo._graph = None
        sampler.shutdown()
    assert used[0] > 0 and used[1] == 0, used
    assert len(outs[0]) == len(outs[1]) and len(outs[0]) > 6
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][3]) > 0


# ---- refusals

@gpu
def test_bits_that_cannot_be_served_are_refused():
    """C % 32 != 0 -> ARL_E_RANGE, a pointer off its 4-byte alignment -> ARL_E_ALIGN, bits without the f32 mask ->
    ARL_E_ARG; a split reduction and the fp32 route's kernels -> ARL_E_RANGE.  Nothing is launched, nothing ignored."""
    from accel_rl_amd import _lib
    lib = _lib.load()
    E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
    sp = _lib.stream_ptr()
    ws = workspace()
    bits = torch.full((4096,), FILL, dtype=torch.int32, device=DEV)

    # forward: 48 filters (C % 32 != 0), a misaligned pointer
    g48 = _lib.conv_geom(2, 12, 9, 64, 48, 3, 3, 1, 1, 1)
    x, w48, y48 = randn((2, 12, 9, 64), 1), randn((48, 3, 3, 64), 2), torch.full((2 * 108, 48), 5.0, device=DEV)
    fwd = lambda g, w, y, p: lib.arl_conv2d_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), p, C.byref(g), 1,  # noqa: E731
                                                ws.data_ptr(), None, sp)
    assert fwd(g48, w48, y48, bits.data_ptr()) == E_RANGE
    g64 = geom_of(CONV3, 2)
    w64, y64 = randn((64, 3, 3, 64), 3), torch.full((2 * 108, 64), 5.0, device=DEV)
    assert fwd(g64, w64, y64, bits.data_ptr() + 2) == E_ALIGN
    assert fwd(g64, w64, y64, bits.data_ptr() + 1) == E_ALIGN
    # the fp32 route's 64-column kernel (16-wide tiles) and a dense layer whose reduction is split write no bits
    g64f = _lib.conv_geom(2, 12, 9, 64, 64, 3, 3, 1, 1, 1, route=_lib.ROUTE_FP32)
    assert fwd(g64f, w64, y64, bits.data_ptr()) == E_RANGE
    gd = _lib.dense_geom(4, 6912, 512)
    xd, wd, yd = randn((4, 6912), 4), randn((512, 6912), 5), torch.full((4, 512), 5.0, device=DEV)
    assert _lib.conv2d_fwd_plan(gd)[0] > 1
    assert lib.arl_conv2d_fwd(xd.data_ptr(), wd.data_ptr(), None, yd.data_ptr(), bits.data_ptr(), C.byref(gd), 1,
                              ws.data_ptr(), None, sp) == E_RANGE
    # u8 forward: 16 filters
    g16 = _lib.conv_geom(1, 104, 80, 4, 16, 8, 8, 4, 0, 0)
    obs = torch.zeros((1, 4, 104, 80), dtype=torch.uint8, device=DEV)
    w16, y16 = randn((16, 4, 8, 8), 6), torch.full((475, 16), 5.0, device=DEV)
    u8 = lambda g, w, y, p: lib.arl_conv2d_u8_fwd(obs.data_ptr(), 1, None, 1.0, w.data_ptr(), None, y.data_ptr(), p,  # noqa: E731
                                                  C.byref(g), 1, sp)
    assert u8(g16, w16, y16, bits.data_ptr()) == E_RANGE
    w32, y32 = randn((32, 4, 8, 8), 7), torch.full((475, 32), 5.0, device=DEV)
    assert u8(geom_of(CONV1, 1), w32, y32, bits.data_ptr() + 2) == E_ALIGN
    # data gradient: 48 input channels, a misaligned pointer, bits without the mask
    g48i = _lib.conv_geom(2, 12, 9, 48, 64, 3, 3, 1, 1, 1)
    dy, wi, m48, dx48 = randn((2, 12, 9, 64), 8), randn((64, 3, 3, 48), 9), randn((216, 48), 10), torch.full((216, 48), 5.0, device=DEV)
    bwd = lambda g, w, m, dx, p: lib.arl_conv2d_bwd_data(dy.data_ptr(), w.data_ptr(), None, m, p, dx.data_ptr(),  # noqa: E731
                                                         C.byref(g), None, None, sp)
    assert bwd(g48i, wi, m48.data_ptr(), dx48, bits.data_ptr()) == E_RANGE
    m64, dx64 = randn((216, 64), 11), torch.full((216, 64), 5.0, device=DEV)
    assert bwd(g64, w64, m64.data_ptr(), dx64, bits.data_ptr() + 2) == E_ALIGN
    assert bwd(g64, w64, None, dx64, bits.data_ptr()) == E_ARG
    # the pair
    item, plan = _lib.ArlFoldItem(), _lib.ArlWgradPlan()
    dw = torch.zeros_like(w64)
    pair = lambda p: lib.arl_conv2d_bwd_pair(dy.data_ptr(), w64.data_ptr(), None, m64.data_ptr(), p, dx64.data_ptr(),  # noqa: E731
                                             m64.data_ptr(), dw.data_ptr(), C.byref(g64), ws.data_ptr(),
                                             ws.numel() * 4, C.byref(item), None, None, None, None, C.byref(plan), sp)
    assert pair(bits.data_ptr() + 2) == E_ALIGN
    assert b"rectifier bits" in lib.arl_last_error()
    torch.cuda.synchronize()
    for t in (y48, y64, yd, y16, y32, dx48, dx64):
        assert bool((t == 5.0).all())                       # nothing was launched
    assert bool((bits == FILL).all()) and float(dw.abs().sum()) == 0.0
    # and the Python wrappers pass the library's refusal on
    with pytest.raises(RuntimeError, match="rectifier bits"):
        _lib.conv2d_fwd(x, w48, None, y48, g48, True, ws, y_bits=bits)


@gpu
def test_forward_with_an_item_and_bits():
    """arl_conv2d_fwd given both item_or_null and y_bits_or_null (bf16-split route).  A layer that does not split (2 x 9 x
    9 x 32, 64 filters of 4 x 4, stride 2: 18 rows) reports splits == 0 and writes the y and the words of the call without
    an item; a split reduction (64 x 6912 -> 512) is refused with ARL_E_RANGE and nothing is launched."""
    from accel_rl_amd import _lib
    lib = _lib.load()
    sp, ws = _lib.stream_ptr(), workspace()
    rows, ch = 18, 64
    g = _lib.conv_geom(2, 9, 9, 32, ch, 4, 4, 2, 0, 0, route=_lib.ROUTE_SPLIT9)
    x, w, bias = randn((2, 9, 9, 32), 41), randn((ch, 4, 4, 32), 42, 0.05), randn((ch,), 43, 0.1)

    def run(item):
        y = torch.full((rows, ch), -7.0, device=DEV)
        buf, bits = guarded(rows * ch // 32)
        assert lib.arl_conv2d_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), bits.data_ptr(), C.byref(g), 1,
                                  ws.data_ptr(), item, sp) == 0
        return y, buf, bits
    item = _lib.ArlFoldItem(splits=-5)
    y1, buf1, bits1 = run(C.byref(item))
    assert item.splits == 0
    assert len(_lib.conv_launch_log()) == 1
    y0, _, bits0 = run(None)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(bits0, bits1)
    check_words(buf1, bits1, y1, ch)
    # a reduction that splits: the fold would have to write the bits
    gd = _lib.dense_geom(64, 6912, 512, route=_lib.ROUTE_SPLIT9)
    assert _lib.conv2d_fwd_plan(gd)[0] > 1
    xd, wd, yd = randn((64, 6912), 44), randn((512, 6912), 45, 0.02), torch.full((64, 512), 5.0, device=DEV)
    buf, bits = guarded(64 * 512 // 32)
    assert lib.arl_conv2d_fwd(xd.data_ptr(), wd.data_ptr(), None, yd.data_ptr(), bits.data_ptr(), C.byref(gd), 1,
                              ws.data_ptr(), C.byref(item), sp) == -2
    assert b"rectifier bits" in lib.arl_last_error() and _lib.conv_launch_log() == []
    torch.cuda.synchronize()
    assert bool((yd == 5.0).all()) and bool((buf == FILL).all())
