"""NGU on the device: arl_epi_knn and arl_epi_mix against the restatements of tests/ngu_ref.py, bit for bit over three
calls that carry their state; arl_invdyn_loss_parts and NguEmbedding.loss_and_grads against float64 autograd; the
refusals; NguPPO / NguA2C on the synthetic env -- replayed against eager, the bonus switched off against plain PPO."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ngu_ref
import rnd_ref
from test_head_limits_gpu import _nan, _untouched
from test_ppg_gpu import _assert_same_run, _whole_step_close
from test_rnd_gpu import DEV, PPO_ARGS, RND_ARGS, _dev, _embed64, _nan64, _rollout, _same_bits, _train

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
# n_env, horizon, M, k, E: the issue's four, and one with more than 64 candidates before a row (several staged tiles, a
# ring of 130 that is full and wraps from the second call on)
SHAPES = [(1, 1, 1, 1, 4), (3, 7, 4, 3, 4), (2, 5, 3, 5, 36), (5, 6, 64, 10, 128), (2, 70, 130, 16, 4)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _three_rollouts(shape):
    """[(emb, dones)] x 3.  Env 0: a done in the first row of call 0, in the middle of call 1, in the last row of call 2;
    the last env (when there are several) never has one; the others draw theirs.  Every call repeats an embedding
    (row 1 = row 0) and call 1 repeats the last one of call 0, across the carried ring."""
    n, t, m, k, e = shape
    rs = np.random.RandomState(sum(shape))
    calls, prev = [], None
    for call in range(3):
        emb = rs.randn(n, t, e).astype(F32)
        dones = (rs.rand(n, t) < 0.2).astype(np.uint8)
        dones[0] = 0
        if t > 1 or call == 0:                      # (one row per call: a done in call 0 alone, so that later rows search)
            dones[0, (0, t // 2, t - 1)[call]] = 1
        if n > 1:
            dones[n - 1] = 0
        if t > 1:
            emb[:, 1] = emb[:, 0]
        if prev is not None:
            emb[:, 0] = prev[:, t - 1]
        calls.append((emb, dones))
        prev = emb
    return calls


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def knn_calls(request, L):
    """Three consecutive arl_epi_knn calls on the device and by the restatement: [(got, want)] per call, each (knn, m,
    mem, n_ins), plus whether every guard band kept its fill."""
    n, t, m, k, e = shape = request.param
    mem, n_ins = _nan(n + 2, m, e), torch.zeros(n + 2, dtype=torch.int32, device=DEV)
    mem[1:n + 1] = 0.
    ref_mem, ref_ins = np.zeros((n, m, e), F32), np.zeros(n, np.int32)
    out, clean = [], True
    for emb, dones in _three_rollouts(shape):
        knn, cnt = _nan64((n * t + 2) * k), torch.full((n * t + 2,), -7, dtype=torch.int32, device=DEV)
        L.epi_knn(_dev(emb), _dev(dones), n, t, mem[1:n + 1], n_ins[1:n + 1], k, knn[k:(n * t + 1) * k], cnt[1:n * t + 1])
        torch.cuda.synchronize()
        clean = clean and all(_untouched(x) for x in (knn[:k], knn[-k:], mem[0], mem[-1])) and \
            cnt[0].item() == cnt[-1].item() == -7 and n_ins[0].item() == n_ins[-1].item() == 0
        w_knn, w_m, ref_mem, ref_ins = ngu_ref.knn(emb, dones, ref_mem, ref_ins, k)
        got = (knn[k:(n * t + 1) * k].view(n * t, k).cpu().numpy(), cnt[1:n * t + 1].cpu().numpy(),
               mem[1:n + 1].cpu().numpy(), n_ins[1:n + 1].cpu().numpy())
        out.append((got, (w_knn, w_m, ref_mem.copy(), ref_ins.copy()), dones))
    return shape, out, clean


def test_knn_three_calls_bit_for_bit(knn_calls):
    shape, calls, clean = knn_calls
    n, t, m, k, e = shape
    assert clean
    for call, (got, want, dones) in enumerate(calls):
        for g, w, what in zip(got, want, ("knn", "m", "mem", "n_ins")):
            if w.dtype == np.int32:
                assert np.array_equal(g, w), (what, call, g, w)
            else:
                _same_bits(g, w, "%s %d" % (what, call))
    # what the cases must contain
    every_m = np.concatenate([w[1] for _, w, _ in calls])
    every_d = np.concatenate([w[0].reshape(-1) for _, w, _ in calls])
    assert calls[0][2][0, 0] and (t == 1 or (calls[1][2][0, t // 2] and calls[2][2][0, t - 1]))
    assert (every_m < k).any() and every_m.max() == min(k, m, 3 * t - 1)
    assert (every_d == 0).any()                                     # the duplicated embedding
    if n > 1:
        assert not any(d[n - 1].any() for _, _, d in calls) and calls[2][1][3][n - 1] == 3 * t
    if shape == (2, 5, 3, 5, 36):
        assert m < t and (calls[0][1][1].reshape(n, t)[n - 1] == [0, 1, 2, 3, 3]).all()     # the ring wraps inside a rollout


@pytest.mark.parametrize("with_err", [True, False], ids=["err", "noerr"])
def test_mix_three_calls_bit_for_bit(L, knn_calls, with_err):
    """On the distances of the three knn calls; the last call has the bonus switched off and returns r_ext's bits."""
    shape, calls, _ = knn_calls
    n, t, m, k, e = shape
    rows = n * t
    rs = np.random.RandomState(rows + with_err)
    dist, mom = _nan64(4), _nan64(5)
    dist[1:3], mom[1:4] = 0., 0.
    ref_dist, ref_mom = np.zeros(2), np.zeros(3)
    par = dict(eps=1e-3, c=1e-3, xi=8e-3, s_max=8., mod_clip=5.)
    for call, (c_ext, c_int) in enumerate(((2., 1.), (2., 0.5), (1., 0.))):
        knn_d, cnt = calls[call][1][0], calls[call][1][1]
        err = (rs.rand(rows) * 2).astype(F32) if with_err else None
        r_ext = rs.randn(rows).astype(F32)
        r_ext[0] = F32(-0.0)
        r_mix, diag = _nan(rows + 2), _nan(5)
        L.epi_mix(_dev(knn_d), _dev(cnt), None if err is None else _dev(err), _dev(r_ext), dist[1:3], mom[1:4], par["eps"],
                  par["c"], par["xi"], par["s_max"], par["mod_clip"], c_ext, c_int, r_mix[1:rows + 1], diag[1:4])
        torch.cuda.synchronize()
        want, ref_dist, ref_mom, want_diag = ngu_ref.mix(knn_d, cnt, err, r_ext, ref_dist, ref_mom, c_ext=c_ext,
                                                         c_int=c_int, **par)
        _same_bits(r_mix[1:rows + 1].cpu().numpy(), want, "r_mix %d" % call)
        _same_bits(dist[1:3].cpu().numpy(), ref_dist, "dist_mean %d" % call)
        _same_bits(mom[1:4].cpu().numpy(), ref_mom, "err_moments %d" % call)
        _same_bits(diag[1:4].cpu().numpy(), want_diag, "diag %d" % call)
        assert all(_untouched(x[:1]) and _untouched(x[-1:]) for x in (r_mix, diag, dist, mom))
        if call == 2:
            _same_bits(r_mix[1:rows + 1].cpu().numpy(), r_ext, "the bonus switched off")
        elif rows > 1:
            assert not np.array_equal(want, (c_ext * r_ext.astype(F64)).astype(F32))
    assert ref_mom[0] == (3 * rows if with_err else 0)


KNN_ARGS = ("emb", "dones", "n_env", "horizon", "width", "memory_size", "k", "mem", "n_ins", "knn", "m")
MIX_ARGS = ("knn", "m", "err", "r_ext", "rows", "k", "dist", "mom", "eps", "c", "xi", "s_max", "mod_clip", "c_ext", "c_int",
            "r_mix", "diag")
REFUSALS = [("knn", k, v, -2) for k, v in (("width", 0), ("width", 6), ("width", 132), ("memory_size", 0),
                                           ("memory_size", 4097), ("k", 0), ("k", 17), ("horizon", 0), ("horizon", 4097),
                                           ("n_env", 0), ("n_env", 65536))]
REFUSALS += [("mix", k, v, -2) for k, v in (("rows", 0), ("rows", (1 << 22) + 1), ("k", 0), ("k", 17))]
REFUSALS += [("mix", k, v, -1) for k, v in (("eps", 0.), ("c", -1.), ("xi", float("nan")), ("s_max", 0.), ("mod_clip", 0.5),
                                            ("c_int", float("inf")), ("dist", None), ("r_mix", "r_ext"))]
REFUSALS += [("knn", "emb", None, -1), ("knn", "m", None, -1), ("knn", "mem", 4, -3), ("knn", "knn", 4, -3),
             ("knn", "n_ins", 2, -3), ("knn", "m", 2, -3), ("knn", "all_rows", None, -2),
             ("mix", "dist", 4, -3), ("mix", "r_mix", 2, -3), ("mix", "err", 2, -3)]
INV_ARGS = ("e", "w1", "b1", "w2", "b2", "actions", "weight", "batch", "width", "hidden", "n_actions", "de", "dw1", "db1",
            "dw2", "db2", "loss2", "ws", "items")
REFUSALS += [("inv", k, v, -2) for k, v in (("width", 0), ("width", 6), ("width", 132), ("hidden", 0), ("hidden", 6),
                                            ("hidden", 260), ("blocks", None), ("n_actions", 1), ("n_actions", 65),
                                            ("batch", 0), ("batch", (1 << 24) + 1))]
REFUSALS += [("inv", "w2", None, -1), ("inv", "de", None, -1), ("inv", "e", 4, -3), ("inv", "dw1", 4, -3), ("inv", "b1", 2, -3)]


@pytest.mark.parametrize("fn,name,value,code", REFUSALS, ids=["%s-%s-%s" % r[:3] for r in REFUSALS])
def test_refusals_leave_the_fill(L, fn, name, value, code):
    """Each limit one step outside, a NULL pointer (value None), a pointer moved off its alignment (value = bytes), r_mix
    aliasing r_ext: the documented code, and every output keeps its fill."""
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=DEV)                      # noqa: E731
    if fn == "inv":     # width 8, hidden 8, 3 actions, 2 pairs
        t = dict(e=_nan(4, 8), w1=_nan(128), b1=_nan(8), w2=_nan(24), b2=_nan(4), weight=_nan(2), de=_nan(4, 8), dw1=_nan(128),
                 db1=_nan(8), dw2=_nan(24), db2=_nan(4), loss2=_nan(4), ws=_nan(1 << 16),
                 actions=torch.zeros(2, dtype=torch.uint8, device=DEV))
        a, outs = dict(batch=2, width=8, hidden=8, n_actions=3, items=None), ("de", "dw1", "db1", "dw2", "db2", "loss2", "ws")
    elif fn == "knn":
        t = dict(emb=_nan(6, 8), dones=torch.zeros(6, dtype=torch.uint8, device=DEV), mem=_nan(65), n_ins=i32(2, -7),
                 knn=_nan64(13), m=i32(6, -7))
        a, outs = dict(n_env=2, horizon=3, width=8, memory_size=4, k=2), ("mem", "knn")
    elif fn == "mix":
        t = dict(knn=torch.ones(8, dtype=torch.float64, device=DEV), m=i32(4, 1), err=torch.ones(4, device=DEV),
                 r_ext=torch.ones(5, device=DEV), dist=_nan64(3), mom=_nan64(3), r_mix=_nan(5), diag=_nan(3))
        a, outs = dict(rows=4, k=2, eps=1e-3, c=1e-3, xi=8e-3, s_max=8., mod_clip=5., c_ext=1., c_int=1.), \
            ("dist", "mom", "r_mix", "diag")
    a.update({k: v.data_ptr() for k, v in t.items()})
    if name == "all_rows":                  # n_env * horizon one step past 2^24, each inside its own limit
        a.update(n_env=4097, horizon=4096)
    elif name == "blocks":                  # ceil(2 width / 32) ceil(hidden / 32) = 8 * 3 > 16
        a.update(width=128, hidden=68)
    elif name in t:
        a[name] = None if value is None else a[value] if isinstance(value, str) else a[name] + value
    else:
        a[name] = value
    lib = L.load()
    entry, order = dict(knn=(lib.arl_epi_knn, KNN_ARGS), mix=(lib.arl_epi_mix, MIX_ARGS),
                        inv=(lib.arl_invdyn_loss_parts, INV_ARGS))[fn]
    assert entry(*[a[k] for k in order], L.stream_ptr()) == code
    torch.cuda.synchronize()
    assert all(_untouched(t[x]) for x in outs)
    assert fn != "knn" or ((t["m"] == -7).all() and (t["n_ins"] == -7).all())


# ---- arl_invdyn_loss_parts -----------------------------------------------------------------------------------------------

def _head64(e, w1, b1, w2, b2, actions, weight):
    """loss, accuracy of the head in float64 torch: e [2B, E] read as [B, 2E]"""
    logits = F.relu(e.reshape(actions.shape[0], -1) @ w1 + b1) @ w2 + b2
    ce = F.cross_entropy(logits, actions, reduction="none")
    denom = weight.sum().clamp(min=1.0)
    return (weight * ce).sum() / denom, (weight * (logits.argmax(1) == actions)).sum() / denom


# B: one below the row tile of 32 pairs, the tile, one over, two tiles + 1; an all-masked batch once per size
HEAD_CASES = [(b, s, False) for s in ((4, 4, 2), (32, 128, 18)) for b in (31, 32, 33, 65)]
HEAD_CASES += [(33, (4, 4, 2), True), (33, (32, 128, 18), True)]


@pytest.mark.parametrize("b,sizes,masked", HEAD_CASES, ids=["%d-%s%s" % (b, "x".join(map(str, s)), "-allmasked" * m)
                                                            for b, s, m in HEAD_CASES])
def test_invdyn_head_against_float64_autograd(L, b, sizes, masked):
    e_w, h_w, n_act = sizes
    rs = np.random.RandomState(b + e_w)
    host = [rs.randn(2 * b, e_w), rs.randn(2 * e_w, h_w) / np.sqrt(2 * e_w), rs.randn(h_w) * 0.1,
            rs.randn(h_w, n_act) / np.sqrt(h_w), rs.randn(n_act) * 0.1]
    actions = rs.randint(0, n_act, size=b)
    weight = np.zeros(b) if masked else (rs.rand(b) < 0.7).astype(F64)
    dev = [_dev(a.astype(F32)) for a in host]
    outs = [_nan(*a.shape) for a in host] + [_nan(4)]
    L.invdyn_loss(*dev, _dev(actions.astype(np.uint8)), _dev(weight.astype(F32)), *outs,
                  L.invdyn_workspace(e_w, h_w, n_act, DEV))
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    assert _untouched(outs[5][2:]) and all(np.isfinite(g).all() for g in got[:5]) and np.isfinite(got[5][:2]).all()
    if masked:
        assert all((g == 0).all() for g in got[:5]) and (got[5][:2] == 0).all()
        return
    leaves = [d.cpu().double().requires_grad_() for d in dev]
    loss, acc = _head64(*leaves, torch.from_numpy(actions), torch.from_numpy(weight))
    want = [g.numpy() for g in torch.autograd.grad(loss, leaves)]
    assert 0 < weight.sum() < b and abs(got[5][0] - loss.item()) <= 2e-3 * loss.item()
    assert abs(got[5][1] - acc.item()) <= 1e-6
    scale = max(np.abs(g).max() for g in want)
    for g, wv, what in zip(got, want, ("de", "dW1", "db1", "dW2", "db2")):
        assert np.abs(wv).max() > 0, what
        _whole_step_close(g, wv, scale, "B %d %s" % (b, what))


@functools.lru_cache(maxsize=None)
def _embedding_setup():
    from accel_rl_amd.policies.ngu_network import NguEmbedding
    from accel_rl_amd.policies.rnd_network import RndNetwork
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    spec = EnvSpec(UintBox((4, 104, 80)), Discrete(6))
    rnd = RndNetwork(embedding_size=64, predictor_hidden=(64,), rnd_seed=4)
    rnd.initialize(spec, 4, device=DEV)
    net = NguEmbedding(rnd, embedding_size=16, head_hidden=32, seed=2)
    net.initialize(spec, 4, 8, device=DEV)
    obs, extra = (_dev(a) for a in _rollout(np.random.RandomState(12), 4, 2, 4, 104, 80))
    rnd.update_obs_stats(obs, extra)
    return rnd, net, obs, extra


@pytest.mark.parametrize("b", [3, 8])
def test_embedding_gradient_matches_float64_autograd(b):
    """4 envs x horizon 2.  Row 4 is the first of its env's rollout, row 3 has a done: both pairs weigh 0; so does row 7,
    whose pair (6, 7) holds the done row 6."""
    rnd, net, obs, extra = _embedding_setup()
    idx = None if b == 8 else _dev(np.array([5, 4, 3], dtype=np.int32))
    rows = np.arange(8) if idx is None else idx.cpu().numpy()
    actions, dones = np.array([0, 1, 2, 3, 4, 5, 0, 1]), np.array([0, 0, 0, 1, 0, 0, 1, 0], np.uint8)
    net.flat_grads.fill_(float("nan"))
    loss2 = net.loss_and_grads(obs, extra, idx, _dev(actions), _dev(dones)).cpu().numpy()
    got = [g.detach().cpu().numpy().copy() for g in net.grads]
    before = np.maximum(rows - 1, 0)
    weight = ((rows % 2 != 0) & (dones[rows] == 0) & (dones[before] == 0)).astype(F64)
    assert weight.tolist() == ([1, 0, 0] if b == 3 else [0, 1, 0, 0, 0, 1, 0, 0])
    frames = rnd_ref.next_frames(obs.cpu().numpy(), extra.cpu().numpy(), 4, 2)[np.stack((before, rows), 1).reshape(-1)]
    st = rnd.rnd_state()
    x64 = torch.from_numpy(rnd_ref.obs_prepare(frames, st["obs_count"][0], st["obs_mean"], st["obs_m2"])).double()
    params = [p.detach().cpu().double().requires_grad_() for p in net.params]
    emb = _embed64(net, params[:-4], x64.permute(0, 3, 1, 2))
    loss, acc = _head64(emb, *params[-4:], torch.from_numpy(actions[rows]), torch.from_numpy(weight))
    want = [g.numpy() for g in torch.autograd.grad(loss, params)]
    assert abs(loss2[0] - loss.item()) <= 2e-3 * loss.item() and abs(loss2[1] - acc.item()) <= 1e-6
    scale = max(max(np.abs(g).max() for g in want), 1e-3)
    assert all(np.isfinite(g).all() for g in got)
    for k, (g, wv) in enumerate(zip(got, want)):
        assert np.abs(wv).max() > 0, k
        _whole_step_close(g, wv, scale, "B %d param %d" % (b, k))


# ---- the algorithms --------------------------------------------------------------------------------------------------------

NGU_KW = dict(rnd_args=RND_ARGS, ngu_args=dict(embedding_size=16, head_hidden=32, seed=5), memory_size=8, k=3)
NGU_KEYS = ["EpiRewMean", "GradNorm", "InvDynAcc", "InvDynLoss", "ModMean", "RndLoss"]


def _ngu(name):
    from accel_rl_amd.algos import pg
    return getattr(pg, name)


def test_ngu_ppo_replayed_iterations_equal_eager_ones():
    """Six iterations: two eager, one captured, three replayed; the same seeded run made eagerly ends in the same policy,
    the same memories and moments, and returned the same diagnostics, bit for bit.  horizon 5 < 8 slots < 25 steps of an
    episode < the run's 30 steps: the rings fill, wrap, and are cleared at a done."""
    kw = dict(rnd_rows_per_pass=16, **NGU_KW, **PPO_ARGS)
    algo, policy, log = _train(_ngu("NguPPO"), True, 6, **kw)
    assert algo._graph is not None and len(log["infos"]) == 6
    for info in log["infos"]:
        assert sorted(info) == NGU_KEYS and all(np.isfinite(v).all() for v in info.values())
        assert 1 <= info["ModMean"][0] <= 5 and info["EpiRewMean"][0] > 0 and info["InvDynLoss"][0] > 0
    algo_e, policy_e, log_e = _train(_ngu("NguPPO"), False, 6, **kw)
    assert algo_e._graph is None
    _assert_same_run(log, policy, log_e, policy_e)
    state, state_e = algo.ngu.ngu_state(), algo_e.ngu.ngu_state()
    for key in state:
        assert np.array_equal(state[key].view(np.uint8), state_e[key].view(np.uint8)), key
    assert algo._ngu_opt._step_count.item() == 6 * 4
    assert state["err_moments"][0] == 6 * 40 and state["n_ins"].min() >= 1 and state["n_ins"].max() < 6 * 5
    assert np.array_equal(algo.rnd.rnd_state()["predictor"].view(np.uint32),
                          algo_e.rnd.rnd_state()["predictor"].view(np.uint32))


def test_ngu_ppo_with_the_bonus_switched_off_is_plain_ppo():
    from accel_rl_amd.algos.pg.ppo import PPO
    algo, policy, log = _train(_ngu("NguPPO"), True, 4, int_coeff=0., ext_coeff=1., **NGU_KW, **PPO_ARGS)
    algo_p, policy_p, log_p = _train(PPO, True, 4, **PPO_ARGS)
    assert np.array_equal(log["first"], log_p["first"])
    _same_bits(policy.get_param_values(), policy_p.get_param_values(), "policy parameters")
    assert not np.array_equal(policy.get_param_values(), log["first"])


def test_ngu_a2c_runs_two_iterations():
    algo, policy, log = _train(_ngu("NguA2C"), True, 2, **NGU_KW)
    assert len(log["infos"]) == 2 and not np.array_equal(policy.get_param_values(), log["first"])
    for info in log["infos"]:
        assert sorted(info) == NGU_KEYS and all(np.isfinite(v).all() for v in info.values())
