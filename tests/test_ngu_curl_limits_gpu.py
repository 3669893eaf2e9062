"""The NGU and CURL kernels at the limits their entry points accept (csrc/episodic.hip, csrc/curl.hip).  The feature tests
(test_ngu_gpu.py, test_curl_gpu.py) stay as they are; this file runs what they leave out:

- arl_curl_loss_parts against float64 autograd of test_curl_gpu._infonce64 under test_curl_gpu._close's bars: batches of
  2048 / 2049 / 4096 (a workgroup's second query tile: one row of it, all of it; dzq of the rows from 2048 on compared on
  their own), widths 8, 12, 32, 64, 68, 100, 124 (every deal-out of the reduction to the four waves, one / three / a
  ragged fourth column block), a row whose maximum arrives with the last key more than 100 above everything before it
  (the rescale underflows to 0), the diagonal in the last key tile, a row of the ragged last query tile, exact ties
  between bitwise equal keys (the FIRST arg-max), coef < 0 and coef = 1e-30, two launches the same bits at 4096 x 128,
  and every refusal with the outputs and the workspace left at their fill;
- arl_invdyn_loss_parts against float64 autograd of test_ngu_gpu._head64 under that file's bars: n_actions 32, 33, 64
  (the second logits block, the strides A | 1 and 65), sizes that are no multiple of 32, both corners of the 16-block
  limit, hidden 256 at the largest n_actions the LDS takes and the refusal one above it, 2048 / 2049 / 4097 pairs (the
  second and third tile of a workgroup, de of those pairs compared on its own), fractional weights that sum to 0.3 and
  1.7, action bytes n_actions and 255, a batch whose only weighted pair is its last;
- arl_epi_knn bit for bit against ngu_ref.knn_fast over carried calls: dones past one trip of both done scans, horizon
  and memory_size 4096 (sixteen nearest neighbours that all pass through one lane, twenty bitwise duplicates), a ring of 5
  under 4096 rows and one of 4096 over 27, widths 28 and 32, 65535 environments, counts planted at and past 2^30;
- arl_epi_mix bit for bit against ngu_ref.mix: 1024 / 1025 / 3000 rows (a thread's second and third row) at k = 16 and 1,
  no valid distance at all, m above k, a running mean of 0 and of 1e-12 under the 1e-8 clamp, s on both sides of s_max,
  both ends of the modulator clip, a xi that zeroes every dn.

tests/test_ngu_curl_limits_host.py proves, without a GPU, that every case holds what it is named for.  Every output
lies inside a larger buffer filled with NaN (integers: -7) whose excess must stay untouched.

Every fp32 test prints max |err| / max |want| per output before it asserts.  Measured on an MI355X under the feature
tests' bars, which stand unchanged (gradients rtol 2e-3 and atol 2e-5 max |want|, losses 2e-3 relative, accuracy exact or
1e-6): CURL at 4096 x 128 dzq 1.6e-6, dw 1.1e-6; at 4096 x 4 dzq 9.9e-6, dw 7.1e-7; the planted rows dzq 1.1e-6, dw 3.5e-7;
every loss within 2e-7 relative.  The head at 2048 .. 4097 pairs: every gradient within 1.7e-7 of the scale, loss 1.1e-7
relative, accuracy within 6e-8.  The 64 times longer accumulation costs nothing that the bars could see."""
import functools

import numpy as np
import pytest
import torch

import curl_ref as cr
import ngu_ref
from test_curl_gpu import _close, _infonce64
from test_ngu_gpu import INV_ARGS, _head64
from test_ppg_gpu import _whole_step_close
from test_rnd_gpu import _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F32, F64 = np.float32, np.float64
PAD = 64                                                        # guard elements behind every output
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _guarded(shape, fill=NAN, dtype=torch.float32, init=None):
    """-> (the whole buffer, its leading view of `shape`): the view is what a kernel is given."""
    n = int(np.prod(shape))
    big = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
    view = big[:n].view(shape)
    if init is not None:
        view.copy_(_dev(init))
    return big, view


def _tail_untouched(big, n, fill=NAN):
    tail = big[n:]
    assert tail.numel() >= PAD
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def _rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


# ---- arl_curl_loss_parts -----------------------------------------------------------------------------------------------------

COEF = 0.7


@functools.lru_cache(maxsize=None)
def _curl_want(kind, b, d, coef):
    """(loss, dzq, dw) by float64 autograd, once per case"""
    zq, zk, w, _ = getattr(cr, kind + "_case")(b, d)
    tq, tw = torch.from_numpy(zq).double().requires_grad_(), torch.from_numpy(w).double().requires_grad_()
    loss, _ = _infonce64(tq, torch.from_numpy(zk).double(), tw, coef)
    loss.backward()
    return loss.item(), tq.grad.numpy(), tw.grad.numpy()


def _curl_launch(L, zq, zk, w, coef):
    b, d = zq.shape
    ws_n = L.load().arl_curl_workspace_bytes(d) // 4
    bigs = [_guarded(s) for s in ((b, d), (d, d), (4,), (ws_n,))]
    (dzq, dw, loss2, ws) = [v for _, v in bigs]
    L.curl_loss(_dev(zq), _dev(zk), _dev(w), coef, dzq, dw, loss2, ws)
    torch.cuda.synchronize()
    for (big, v) in bigs:
        assert _tail_untouched(big, v.numel())
    assert torch.isnan(loss2[2:]).all()
    return _host(dzq), _host(dw), _host(loss2[:2])


def _curl_check(L, kind, b, d, coef=COEF):
    zq, zk, w, s = getattr(cr, kind + "_case")(b, d)
    loss, w_dzq, w_dw = _curl_want(kind, b, d, coef)
    dzq, dw, loss2 = _curl_launch(L, zq, zk, w, coef)
    what = "%s B %d D %d" % (kind, b, d)
    print("%s: max|err| / max|want|  dzq %.3g  dw %.3g  loss %.3g (bars: 2e-3 relative, 2e-5 of max|want|)" % (
        what, _rel(dzq, w_dzq), _rel(dw, w_dw), abs(loss2[0] - loss) / abs(loss)))
    assert np.isfinite(dzq).all() and np.isfinite(dw).all() and np.isfinite(loss2).all()
    assert np.abs(w_dzq).max() > 0 and np.abs(w_dw).max() > 0
    _close(dzq, w_dzq, what + " dzq")
    _close(dw, w_dw, what + " dw")
    assert abs(loss2[0] - loss) <= 2e-3 * abs(loss), (what, loss2[0], loss)
    n_hits = cr.hits(s)
    assert round(float(loss2[1]) * b) == n_hits and abs(loss2[1] - n_hits / b) < 1e-6, (what, loss2[1] * b, n_hits)
    return dzq, dw, loss2, w_dzq


@pytest.mark.parametrize("b,d", [(2048, 4), (2049, 4), (4096, 4), (2049, 128), (4096, 128)])
def test_curl_a_workgroups_second_query_tile(L, b, d):
    """64 workgroups x 32 rows = 2048: at 2048 every workgroup makes one trip, at 2049 workgroup 0's second tile holds
    one row, at 4096 every workgroup makes two.  The rows of the second trip are compared on their own."""
    dzq, _, _, want = _curl_check(L, "random", b, d)
    if b > 2048:
        assert np.abs(want[2048:]).max() > 0
        _close(dzq[2048:], want[2048:], "dzq of rows 2048 ..")


@pytest.mark.parametrize("d", [8, 12, 32, 64, 68, 100, 124])
@pytest.mark.parametrize("b", [33, 65])
def test_curl_every_deal_out_of_the_reduction_and_column_block_count(L, b, d):
    _curl_check(L, "random", b, d)


@pytest.mark.parametrize("b,d", [(65, 36), (2049, 36)])
def test_curl_maximum_in_the_last_key_tile_after_an_underflowing_rescale(L, b, d):
    dzq, _, _, want = _curl_check(L, "planted", b, d)
    for row in (cr.PLANTED_ROW, b - 1):
        assert np.abs(want[row]).max() > 0
        _close(dzq[row], want[row], "dzq of row %d" % row)


def test_curl_equal_logits_take_the_first_arg_max(L):
    b, d = 65, 36
    _, _, loss2, _ = _curl_check(L, "tie", b, d)
    s = cr.tie_case(b, d)[3]
    arg = np.argmax(s, axis=1)
    assert [int(arg[r]) for r, _ in cr.TIES] == [min(r, p) for r, p in cr.TIES]
    assert round(float(loss2[1]) * b) == cr.hits(s)             # (the host file: the last arg-max gives two fewer)


def test_curl_negative_and_tiny_coefficients_and_determinism(L):
    b, d = 65, 36
    zq, zk, w, _ = cr.random_case(b, d)
    pos = _curl_launch(L, zq, zk, w, COEF)
    neg = _curl_check(L, "random", b, d, -COEF)[:3]
    for g, h, what in zip(neg, pos, ("dzq", "dw", "loss2")):
        if what == "loss2":
            assert g[0] == -h[0] and g[1] == h[1]
        else:
            assert np.array_equal(g, -h), what                  # coef / B, every product and every sum: the sign alone
    tiny = _curl_check(L, "random", b, d, 1e-30)
    assert all(np.isfinite(x).all() for x in tiny[:3]) and np.abs(tiny[0]).max() > 0
    zq, zk, w, _ = cr.random_case(4096, 128)
    first, again = _curl_launch(L, zq, zk, w, COEF), _curl_launch(L, zq, zk, w, COEF)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(first, again))


CURL_ARGS = ("zq", "zk", "w", "batch", "width", "coef", "dzq", "dw", "loss2", "ws")
CURL_REFUSALS = [(k, v, E_RANGE) for k, v in (("width", 0), ("width", 6), ("width", 132), ("batch", 0), ("batch", 4097))]
CURL_REFUSALS += [("coef", NAN, E_ARG), ("coef", float("inf"), E_ARG), ("coef", -float("inf"), E_ARG)]
CURL_REFUSALS += [(k, None, E_ARG) for k in ("zq", "zk", "w", "dzq", "dw", "loss2", "ws")]
CURL_REFUSALS += [(k, 4, E_ALIGN) for k in ("zq", "zk", "dzq", "dw", "loss2", "ws")] + [("w", 2, E_ALIGN)]


@pytest.mark.parametrize("name,value,code", CURL_REFUSALS, ids=["%s-%s" % r[:2] for r in CURL_REFUSALS])
def test_curl_refusals_leave_outputs_and_workspace_at_their_fill(L, name, value, code):
    """Each limit one step outside, a coefficient that is not finite, a NULL pointer (value None), a pointer moved off its
    alignment (value = bytes): the documented code, and nothing written."""
    lib = L.load()
    t = dict(zq=torch.ones(8, 8, device=DEV), zk=torch.ones(8, 8, device=DEV), w=torch.ones(8, 8, device=DEV),
             dzq=_guarded((8, 8))[0], dw=_guarded((8, 8))[0], loss2=_guarded((4,))[0],
             ws=_guarded((lib.arl_curl_workspace_bytes(8) // 4,))[0])
    a = dict(batch=8, width=8, coef=1.0)
    a.update({k: v.data_ptr() for k, v in t.items()})
    if name in t:
        a[name] = None if value is None else a[name] + value
    else:
        a[name] = value
    assert lib.arl_curl_loss_parts(*[a[k] for k in CURL_ARGS], None, L.stream_ptr()) == code
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[x]).all()) for x in ("dzq", "dw", "loss2", "ws"))


# ---- arl_invdyn_loss_parts ---------------------------------------------------------------------------------------------------

A_MAX = ngu_ref.invdyn_a_max(32, 256)                           # (the host file: 13, from the layout and from the library)
INV_SIZES = [(4, 4, 33), (4, 4, 64), (4, 4, 32), (20, 36, 18), (128, 64, 64), (32, 256, A_MAX)]


def _inv_check(L, b, sizes, second_walk_from=None, **kw):
    e_w, h_w, n_act = sizes
    host, actions, weight = ngu_ref.invdyn_case(b, sizes, **kw)
    dev = [_dev(a.astype(F32)) for a in host]
    ws_n = L.load().arl_invdyn_workspace_bytes(*sizes) // 4
    assert ws_n > 0
    bigs = [_guarded(a.shape) for a in host] + [_guarded((4,)), _guarded((ws_n,))]
    outs = [v for _, v in bigs]
    L.invdyn_loss(*dev, _dev(actions), _dev(weight.astype(F32)), *outs)
    torch.cuda.synchronize()
    for big, v in bigs:
        assert _tail_untouched(big, v.numel())
    got = [_host(o) for o in outs[:6]]
    assert torch.isnan(outs[5][2:]).all() and all(np.isfinite(g).all() for g in got[:5]) and np.isfinite(got[5][:2]).all()
    leaves = [d.cpu().double().requires_grad_() for d in dev]
    read_as = np.minimum(actions.astype(np.int64), n_act - 1)       # the header: a value >= n_actions is n_actions - 1
    loss, acc = _head64(*leaves, torch.from_numpy(read_as), torch.from_numpy(weight))
    want = [g.numpy() for g in torch.autograd.grad(loss, leaves)]
    what = "B %d %s %s" % (b, "x".join(map(str, sizes)), kw or "")
    scale = max(np.abs(g).max() for g in want)
    print("%s: loss %.6g (err %.3g relative, bar 2e-3)  acc %.6g (err %.3g, bar 1e-6)  max|err| / scale %s (bar: 2e-3 "
          "relative, 2e-5 of the scale)" % (what, loss.item(), abs(got[5][0] - loss.item()) / loss.item(), acc.item(),
                                            abs(got[5][1] - acc.item()),
                                            " ".join("%.3g" % (np.abs(g - wv).max() / scale) for g, wv in zip(got, want))))
    assert weight.sum() > 0 and abs(got[5][0] - loss.item()) <= 2e-3 * loss.item(), what
    assert abs(got[5][1] - acc.item()) <= 1e-6, what
    for g, wv, name in zip(got, want, ("de", "dW1", "db1", "dW2", "db2")):
        assert np.abs(wv).max() > 0, name
        _whole_step_close(g, wv, scale, "%s %s" % (what, name))
    if second_walk_from is not None:                                # the pairs a workgroup reaches on its second trip
        lo = 2 * second_walk_from
        assert np.abs(want[0][lo:]).max() > 0 and (weight[second_walk_from:] != 0).all()
        _whole_step_close(got[0][lo:], want[0][lo:], scale, what + " de of the second walk")
    return got, want


@pytest.mark.parametrize("b", [33, 65])
@pytest.mark.parametrize("sizes", INV_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_invdyn_second_logits_block_odd_sizes_and_the_block_limits_corners(L, b, sizes):
    _inv_check(L, b, sizes)


@pytest.mark.parametrize("b,sizes", [(2048, (4, 4, 2)), (2049, (4, 4, 2)), (4097, (4, 4, 2)), (2049, (32, 128, 18))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_invdyn_a_workgroups_second_and_third_tile(L, b, sizes):
    """64 workgroups x 32 pairs: 2048 is one trip each, 2049 gives workgroup 0 a second tile of one pair, 4097 a third."""
    _inv_check(L, b, sizes, second_walk_from=2048 if b > 2048 else None, ones_from=2048)


@pytest.mark.parametrize("kw", [dict(weights="sum0.3"), dict(weights="sum1.7"), dict(over=True), dict(weights="last-only")],
                         ids=["sum0.3", "sum1.7", "actions-over", "last-only"])
@pytest.mark.parametrize("sizes", [(4, 4, 33), (20, 36, 18)], ids=lambda s: "x".join(map(str, s)))
def test_invdyn_edge_inputs(L, sizes, kw):
    _inv_check(L, 65, sizes, **kw)


def test_invdyn_refuses_one_action_past_the_lds_limit(L):
    lib = L.load()
    n_act = A_MAX + 1
    assert lib.arl_invdyn_workspace_bytes(32, 256, n_act) == 0 and lib.arl_invdyn_workspace_bytes(32, 256, A_MAX) > 0
    names = ("de", "dw1", "db1", "dw2", "db2", "loss2", "ws")
    t = dict(e=torch.ones(4, 32, device=DEV), w1=torch.ones(64 * 256, device=DEV), b1=torch.ones(256, device=DEV),
             w2=torch.ones(256 * n_act, device=DEV), b2=torch.ones(n_act, device=DEV), weight=torch.ones(2, device=DEV),
             actions=torch.zeros(2, dtype=torch.uint8, device=DEV), de=_guarded((4, 32))[0], dw1=_guarded((64 * 256,))[0],
             db1=_guarded((256,))[0], dw2=_guarded((256 * n_act,))[0], db2=_guarded((n_act,))[0], loss2=_guarded((4,))[0],
             ws=_guarded((1 << 16,))[0])
    a = dict(batch=2, width=32, hidden=256, n_actions=n_act, items=None)
    a.update({k: v.data_ptr() for k, v in t.items()})
    assert lib.arl_invdyn_loss_parts(*[a[k] for k in INV_ARGS], L.stream_ptr()) == E_RANGE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[x]).all()) for x in names)


# ---- arl_epi_knn -------------------------------------------------------------------------------------------------------------

def _knn_run(L, name):
    """the case's carried calls on the device and by ngu_ref.knn_fast, compared as bits and integers after every call,
    the guard bands included.  -> [(knn, m, mem, n_ins) of the reference per call]"""
    case = ngu_ref.knn_limit_case(name)
    n, t, m, k, e = case["shape"]
    mem_big, mem = _guarded((n, m, e), init=case["mem0"])
    ins_big, n_ins = _guarded((n,), fill=-7, dtype=torch.int32, init=case["ins0"])
    ref_mem, ref_ins = case["mem0"], case["ins0"]
    out = []
    for call, (emb, dones) in enumerate(case["calls"]):
        knn_big, knn = _guarded((n * t, k), dtype=torch.float64)
        cnt_big, cnt = _guarded((n * t,), fill=-7, dtype=torch.int32)
        L.epi_knn(_dev(emb), _dev(dones), n, t, mem, n_ins, k, knn, cnt)
        torch.cuda.synchronize()
        w_knn, w_m, ref_mem, ref_ins = ngu_ref.knn_fast(emb, dones, ref_mem, ref_ins, k)
        what = "%s call %d " % (name, call)
        assert np.array_equal(_host(cnt), w_m), (what + "m", _host(cnt), w_m)
        assert np.array_equal(_host(n_ins), ref_ins), (what + "n_ins", _host(n_ins), ref_ins)
        _same_bits(_host(knn), w_knn, what + "knn")
        _same_bits(_host(mem), ref_mem, what + "mem")
        assert _tail_untouched(knn_big, n * t * k) and _tail_untouched(cnt_big, n * t, -7), what
        assert _tail_untouched(mem_big, n * m * e) and _tail_untouched(ins_big, n, -7), what
        out.append((w_knn, w_m, ref_mem, ref_ins))
    return out


@pytest.mark.parametrize("name", ngu_ref.KNN_LIMIT_NAMES)
def test_knn_carried_calls_bit_for_bit(L, name):
    calls = _knn_run(L, name)
    n, t, m, k, e = ngu_ref.knn_limit_case(name)["shape"]
    every_m = np.concatenate([c[1] for c in calls])
    assert every_m.max() == min(k, m, len(calls) * t - 1)
    if name == "full-4096":                                        # what the host file shows of the reference, of the device
        knn2 = calls[1][0]
        assert knn2[ngu_ref.LANE_ROW].tolist() == [(0.25 * (i + 1)) ** 2 for i in range(16)]
        assert not knn2[ngu_ref.DUP_ROW].any() and calls[1][1][ngu_ref.DUP_ROW] == 16
    if name == "fold":
        assert [c[3].tolist() for c in calls] == [[ngu_ref.FOLD_AT + 4, 11, 3], [12, 15, 7], [16, 19, 11]]


# ---- arl_epi_mix -------------------------------------------------------------------------------------------------------------

def _mix_run(L, k, calls, pars, coefs, dist0, mom0):
    """carried arl_epi_mix calls against ngu_ref.mix (which is given m as the header reads it: at most k), bit for bit"""
    dist_big, dist = _guarded((2,), dtype=torch.float64, init=dist0)
    mom_big, mom = _guarded((3,), dtype=torch.float64, init=mom0)
    ref_dist, ref_mom = dist0.copy(), mom0.copy()
    out = []
    for call, (c, par, (c_ext, c_int)) in enumerate(zip(calls, pars, coefs)):
        rows = c["m"].size
        mix_big, r_mix = _guarded((rows,))
        diag_big, diag = _guarded((3,))
        L.epi_mix(_dev(c["knn"]), _dev(c["m"]), _dev(c["err"]), _dev(c["r_ext"]), dist, mom, par["eps"], par["c"],
                  par["xi"], par["s_max"], par["mod_clip"], c_ext, c_int, r_mix, diag)
        torch.cuda.synchronize()
        before = ref_dist.copy()
        want, ref_dist, ref_mom, want_diag = ngu_ref.mix(c["knn"], np.minimum(c["m"], k), c["err"], c["r_ext"], ref_dist,
                                                         ref_mom, c_ext=c_ext, c_int=c_int, **par)
        _same_bits(_host(r_mix), want, "r_mix %d" % call)
        _same_bits(_host(dist), ref_dist, "dist_mean %d" % call)
        _same_bits(_host(mom), ref_mom, "err_moments %d" % call)
        _same_bits(_host(diag), want_diag, "diag %d" % call)
        assert _tail_untouched(mix_big, rows) and _tail_untouched(diag_big, 3), call
        assert _tail_untouched(dist_big, 2) and _tail_untouched(mom_big, 3), call
        out.append((want, before, ref_dist.copy(), want_diag))
    return out


@pytest.mark.parametrize("with_err", [True, False], ids=["err", "noerr"])
@pytest.mark.parametrize("k", ngu_ref.MIX_LIMIT_K)
@pytest.mark.parametrize("rows", ngu_ref.MIX_LIMIT_ROWS)
def test_mix_a_threads_second_and_third_row(L, rows, k, with_err):
    calls = ngu_ref.mix_rows_case(rows, k, with_err)
    out = _mix_run(L, k, calls, [ngu_ref.MIX_PAR] * 3, ngu_ref.MIX_COEFS, np.zeros(2), np.zeros(3))
    _same_bits(out[2][0], calls[2]["r_ext"], "the bonus switched off")
    assert not np.array_equal(out[0][0], (2. * calls[0]["r_ext"].astype(F64)).astype(F32))


@pytest.mark.parametrize("name", ngu_ref.MIX_PLANTED)
def test_mix_planted_inputs(L, name):
    c = ngu_ref.mix_planted_case(name)
    (r_mix, before, after, diag), = _mix_run(L, c["k"], [c], [c["par"]], [(c["c_ext"], c["c_int"])], c["dist0"], c["mom0"])
    if name == "all-m-zero":                                       # nb == 0: the mean keeps its bits, no bonus anywhere
        _same_bits(after, before, "dist_mean left alone")
        _same_bits(r_mix, (c["c_ext"] * c["r_ext"].astype(F64)).astype(F32), "c_ext r_ext")
        assert diag[0] == 0
    else:
        assert diag[0] > 0
