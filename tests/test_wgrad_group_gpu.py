"""The conv stack's weight gradients as one launch (arl_conv2d_bwd_weight_group over the plans of
arl_conv2d_bwd_weight_parts / arl_conv2d_u8_bwd_weight_parts, csrc/mfma_wgrad.h wgrad_group_kernel) against the separate
launches it replaces (the same two calls with plan_or_null = NULL): the same workgroups doing the same products in the same
order, so EVERYTHING is bit-identical -- dw and dbias after the folds and the raw partial workspaces.

Shapes: the spec-1 layers (conv 1 u8 4 -> 32 8x8 / 4, conv 2 32 -> 64 4x4 / 2 pad 1, conv 3 64 -> 64 3x3 pad 1) at
  B = 1    conv 2 / conv 3: 108 reduction rows, one split, dw written in place (item.splits == 0, no fold); conv 1: 475
  B = 5    ragged last k-tile, a handful of splits
  B = 37   odd; 3 996 rows, tens of splits, a ragged last split
At these three the row count of conv 2 / conv 3 (108 B) is no multiple of the 32-row k-tile, so those two layers run the
generic kernels: the group call has to send them out on their own and keep conv 1's plan intact.  The scalar-addressed
kernels -- the ones that do share the launch -- need 108 B % 32 == 0:
  B = 8    864 rows: 7 splits of 128 rows, the last one ragged (96)
  B = 64   the policy test's size: 6 912 rows, 54 splits, every item more than one group of eight blocks
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = float(np.float32(1. / 255.))
SENTINEL = 7.0
BATCHES = [1, 5, 37, 8, 64]


def _geoms(b, route=None):
    from accel_rl_amd import _lib
    return [_lib.conv_geom(b, 104, 80, 4, 32, 8, 8, 4, 0, 0, route), _lib.conv_geom(b, 25, 19, 32, 64, 4, 4, 2, 1, 1, route),
            _lib.conv_geom(b, 12, 9, 64, 64, 3, 3, 1, 1, 1, route)]


@pytest.fixture(scope="module")
def workspaces():
    """Six conv workspaces (separate / grouped x three layers), allocated once."""
    from accel_rl_amd import _lib
    return [[_lib.conv_workspace(DEV) for _ in range(3)] for _ in range(2)]


@pytest.fixture(scope="module")
def inputs():
    """Per batch size, made once and never written: u8 rows + index list, relu()ed activations, random dy."""
    out = {}
    for b in BATCHES:
        gen = torch.Generator(device=DEV).manual_seed(100 + b)
        obs = torch.randint(0, 256, (b + 3, 4, 104, 80), device=DEV, generator=gen, dtype=torch.int32).to(torch.uint8)
        idx = torch.randint(0, b + 3, (b,), device=DEV, generator=gen, dtype=torch.int32)
        a1 = torch.randn(b, 25, 19, 32, device=DEV, generator=gen).relu()
        a2 = torch.randn(b, 12, 9, 64, device=DEV, generator=gen).relu()
        dys = [torch.randn(b, 25, 19, 32, device=DEV, generator=gen), torch.randn(b, 12, 9, 64, device=DEV, generator=gen),
               torch.randn(b, 12, 9, 64, device=DEV, generator=gen)]
        out[b] = (obs, idx, a1, a2, dys)
    return out


def _run(inp, geoms, layers, ws, grouped):
    """The weight gradients of `layers` (0 = conv 1 ...) separately or as one group; -> per layer (dw, dbias, splits)."""
    from accel_rl_amd import _lib
    obs, idx, a1, a2, dys = inp
    folds = _lib.FoldList()
    res = {}
    for i in layers:
        ws[i].fill_(SENTINEL)
        g = geoms[i]
        dw = torch.full((g.out_c, g.kh * g.kw * g.in_c), SENTINEL, device=DEV)
        db = torch.full((g.out_c,), SENTINEL, device=DEV)
        slot = folds._n
        if i == 0:
            done = folds.conv2d_u8_bwd_weight(dys[0], obs, idx, SCALE, dw, g, ws[0], dbias=db, defer=grouped)
        else:
            done = folds.conv2d_bwd_weight(dys[i], a1 if i == 1 else a2, dw, g, ws[i], dbias=db, defer=grouped)
        res[i] = (dw, db if done else None, folds._items[slot].splits)
    assert folds._n_plans == (len(layers) if grouped else 0)
    folds.run()                                     # the group's launch(es), then the folds
    torch.cuda.synchronize()
    return res


def _same(inp, geoms, layers, workspaces):
    want = _run(inp, geoms, layers, workspaces[0], False)
    got = _run(inp, geoms, layers, workspaces[1], True)
    for i in layers:
        assert want[i][2] == got[i][2], ("splits", i)
        assert torch.isfinite(want[i][0]).all() and not (want[i][0] == SENTINEL).all()
        assert torch.equal(want[i][0], got[i][0]), ("dw", i)
        assert (want[i][1] is None) == (got[i][1] is None)
        if want[i][1] is not None:
            assert torch.equal(want[i][1], got[i][1]), ("dbias", i)
        assert torch.equal(workspaces[0][i], workspaces[1][i]), ("partials", i)
    return want


@pytest.mark.parametrize("route", [9, 6])
@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("layers", [(2, 1, 0), (2, 1), (1,), (0,)], ids=["three", "two", "one", "one_u8"])
def test_group_is_bit_identical_to_separate_launches(b, layers, route, inputs, workspaces):
    from accel_rl_amd import _lib
    geoms = _geoms(b, _lib._PRECISION_TO_ROUTE[route])
    want = _same(inputs[b], geoms, layers, workspaces)
    if b == 1:
        for i in layers:
            if i > 0:
                assert want[i][2] == 0              # one split: dw written in place, nothing to fold
    if b == 37 and 0 in layers:
        assert want[0][2] > 10


@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("odd", [0, 1, 2])
def test_ineligible_item_falls_out_to_its_own_launch(b, odd, inputs, workspaces):
    """One layer on the fp32 route (no group body): launched on its own, the other two as before."""
    from accel_rl_amd import _lib
    geoms = _geoms(b)
    geoms[odd] = _lib.with_route(geoms[odd], _lib.ROUTE_FP32)
    _same(inputs[b], geoms, (2, 1, 0), workspaces)


def _policy_and_minibatch(rows=64):
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(3)
    n, n_act = 96, 4
    policy = AtariCnnPolicy(**cnn_specs[1])
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    rs = np.random.RandomState(11)
    to = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    prob = rs.rand(n, n_act).astype(np.float32) + 0.1
    mb = dict(observations=to(rs.randint(0, 256, size=(n, 4, 104, 80), dtype=np.uint8)),
              idx=to(rs.permutation(n)[:rows].astype(np.int32)), actions=to(rs.randint(0, n_act, size=n).astype(np.uint8)),
              advantages=to(rs.randn(n).astype(np.float32)), returns=to(rs.randn(n).astype(np.float32)),
              old_prob=to(prob / prob.sum(1, keepdims=True)), valids=None)
    return policy, mb


def _grads(policy, mb):
    lr_mult = torch.full((1,), 0.7, device=DEV)
    loss4 = policy.loss_and_grads(mb, 1, 0.2, 1.0, 0.01, lr_mult, None).clone()
    torch.cuda.synchronize()
    return policy.flat_grads.clone(), loss4


@pytest.fixture(params=[9, 6], ids=["split9", "split6"])
def route_policy(request):
    from accel_rl_amd import _lib
    _lib.set_conv_precision(request.param)
    try:
        yield _policy_and_minibatch()
    finally:
        _lib.set_conv_precision(9)


def test_policy_gradients_with_and_without_the_group(route_policy, monkeypatch):
    """policy.loss_and_grads on 64 rows: ARL_WGRAD_GROUP 1 against 0, flat_grads and loss4 bit for bit."""
    policy, mb = route_policy
    monkeypatch.setenv("ARL_WGRAD_GROUP", "0")
    g0, l0 = _grads(policy, mb)
    monkeypatch.setenv("ARL_WGRAD_GROUP", "1")
    g1, l1 = _grads(policy, mb)
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    assert torch.equal(g0, g1) and torch.equal(l0, l1)


def test_policy_gradients_captured_in_a_graph(route_policy, monkeypatch):
    """The same call captured in a torch.cuda.graph and replayed twice: equal to eager."""
    from accel_rl_amd.util.misc import capture_graph
    policy, mb = route_policy
    monkeypatch.setenv("ARL_WGRAD_GROUP", "1")
    want_g, want_l = _grads(policy, mb)             # (also allocates every buffer outside the capture)
    lr_mult = torch.full((1,), 0.7, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        loss4 = policy.loss_and_grads(mb, 1, 0.2, 1.0, 0.01, lr_mult, None)
    for _ in range(2):
        for g in policy.grads:                      # (every gradient tensor; the bucket's padding is never written)
            g.fill_(SENTINEL)
        loss4.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(policy.flat_grads, want_g) and torch.equal(loss4, want_l)
    del graph
