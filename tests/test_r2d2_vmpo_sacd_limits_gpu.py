"""The R2D2, V-MPO (weights) and SAC-Discrete kernels at the limits their entry points accept (csrc/r2d2.hip,
csrc/vmpo.hip, csrc/sac.hip).  The feature tests (test_r2d2_gpu.py, test_vmpo_gpu.py, test_sacd_gpu.py) stay as they are;
this file runs what they leave out:

- arl_seq_store / arl_seq_prepare bit for bit against r2d2_ref.SeqModel: loops past one trip of 256 (horizon 520,
  130 x 256 float4 of state, U = 600), an idx that is no multiple of the stride (t0 != 0; every idx of a small ring), a
  batch that wraps the ring, a full lap, S = 1 and S = horizon = size, no states at all (NULL arrays), hidden = 1024 and
  4, sequences that lap the ring twice, repeated pairs, the last slot of the last environment, block indices above 65535;
- arl_r2d2_loss within one fp32 ulp of r2d2_ref.r2d2_loss64 at train_len = burn_in = 1024 (the whole of the LDS
  arrays), n = 16, A = 255 with and without dueling, the value column in the last float of the row, a block index above
  65535, eta in {0, 1, 0.9}, gamma_n = 0, with a terminal and the largest |d| planted at the last train step;
- arl_vmpo_weights on advantages built from chosen keys: each of the four radix passes the deciding one, the threshold
  in bin 0, in bin 255 and in each of the four bins one lane owns, the two ends of the lane test, the sign change,
  denormals, values up to 0.9 FLT_MAX;
- arl_sacd_loss against float64 within sacd_ref's own bounds over several workgroups and at A = 255 / 253,
  arl_sacd_act at A = 255 over two workgroups, arl_sacd_alpha_grad bit for bit against the stated summation order.

tests/test_r2d2_vmpo_sacd_limits_host.py proves, without a GPU, that every case holds what it is named for.  Every output
lies inside a larger buffer filled with NaN (integers: a sentinel) whose excess must stay untouched."""
import numpy as np
import pytest
import torch

import r2d2_ref as rr
import sacd_ref as sr
import test_sacd_gpu as tsg
import vmpo_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F32 = np.float32
PAD = 64                                                        # guard elements behind every output
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _guarded(shape, fill=NAN, dtype=torch.float32, pad=PAD):
    """-> (the whole buffer, its leading view of `shape`): the view is what a kernel is given."""
    n = int(np.prod(shape))
    big = torch.full((n + pad,), fill, dtype=dtype, device=DEV)
    return big, big[:n].view(shape)


def _tail_untouched(big, n, fill=NAN):
    tail = big[n:]
    assert tail.numel() >= PAD
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


# ---- arl_seq_store ---------------------------------------------------------------------------------------------------------

RING_FILL = 255                                                 # SeqModel's ring starts at 255, its stores at NaN


class _SeqRig(object):
    """SeqModel and its device twin: stores and ring inside guarded buffers, compared as bits after every launch."""

    def __init__(self, n_env, size, S, hidden, n_state):
        self.model = rr.SeqModel(n_env, size, S, hidden, n_state)
        self.n_env, self.size, self.S, self.hidden, self.n_state = n_env, size, S, hidden, n_state
        made = [_guarded((n_env, size // S, hidden)) for _ in range(n_state)]
        self.store_bigs, self.stores = [m[0] for m in made], [m[1] for m in made]
        self.ring_big, self.ring = _guarded((n_env, size), fill=RING_FILL, dtype=torch.uint8)
        self.rs = np.random.RandomState(n_env + 3 * size + 5 * S + hidden + n_state)

    def batch(self, horizon, flag=1):
        states = [self.rs.randn(self.n_env * horizon, self.hidden).astype(F32) for _ in range(self.n_state)]
        for st in states:                                        # -0.0, a denormal, inf: bits, not values
            st.reshape(-1)[:3] = np.array([-0.0, 1e-42, np.inf], F32)
            st.reshape(-1)[-1] = F32(-1e-42)
        resets = (self.rs.rand(self.n_env * horizon) < 0.3).astype(np.uint8) * np.uint8(flag)
        return states, resets

    def store(self, L, horizon, idx, flag=1):
        states, resets = self.batch(horizon, flag)
        self.model.store(states, resets, horizon, idx)
        L.seq_store([_dev(s) for s in states], _dev(resets), self.n_env, horizon, self.size, self.S, idx, self.stores,
                    self.ring)
        self.compare(("store", horizon, idx))

    def compare(self, what):
        torch.cuda.synchronize()
        for big, got, want in zip(self.store_bigs, self.stores, self.model.stores):
            np.testing.assert_array_equal(_bits(_host(got)), _bits(want), err_msg=str(what))
            assert _tail_untouched(big, want.size), what
        np.testing.assert_array_equal(_host(self.ring), self.model.ring, err_msg=str(what))
        assert _tail_untouched(self.ring_big, self.model.ring.size, RING_FILL), what


@pytest.mark.parametrize("n_state", [1, 2])
def test_seq_store_loops_past_one_trip_and_an_idx_off_the_stride(L, n_state):
    """horizon 520: three trips of the reset loop; 130 slots x 256 float4: 130 trips of the state loop; idx 3 and 1037
    give t0 = 1 and 3, and the batch at 1037 wraps the ring."""
    for idx in (0, 3, 1037):
        rig = _SeqRig(2, 1040, 4, 1024, n_state)
        rig.store(L, 520, idx)
        filled = ~np.isnan(rig.model.stores[0][:, :, 0])
        assert (filled.sum(axis=1) == 130).all() and (rig.model.ring != RING_FILL).sum() == 2 * 520
        rig.store(L, 520, (idx + 520) % 1040, flag=2)            # the other half of the ring, from the same offset
        assert not np.isnan(rig.model.stores[0]).any() and (rig.model.ring != RING_FILL).all()


def test_seq_store_at_every_idx_of_a_small_ring(L):
    rig = _SeqRig(3, 40, 8, 8, 2)
    for idx in range(40):
        rig.store(L, 16, idx, flag=1 + idx % 3)
    fresh = _SeqRig(3, 40, 8, 8, 1)                               # on an empty store: exactly two slots per environment
    fresh.store(L, 16, 13)
    assert (~np.isnan(fresh.model.stores[0][:, :, 0])).sum(axis=1).tolist() == [2, 2, 2]


@pytest.mark.parametrize("size,S,horizon,idxs", [(24, 4, 24, (5, 0, 23)), (12, 1, 6, (9, 0, 11)), (16, 16, 16, (0, 7, 15)),
                                                 (1024, 1024, 1024, (1, 1023))])
def test_seq_store_at_the_extremes_of_the_stride(L, size, S, horizon, idxs):
    """a full lap from a non-zero idx; S = 1 (every step stores its state); S = horizon = size (one slot, t0 = S - idx)."""
    for n_state in (1, 2):
        rig = _SeqRig(2, size, S, 4, n_state)
        for idx in idxs:
            rig.store(L, horizon, idx)


def test_seq_store_without_states_changes_only_the_ring(L):
    lib = L.load()
    for size, S, horizon, idx in ((40, 8, 16, 13), (1040, 4, 520, 1037)):
        rig = _SeqRig(2, size, S, 0, 0)
        rig.store(L, horizon, idx)                               # through the wrapper: arrays of no pointers
        _, resets = rig.batch(horizon, flag=3)                   # and with NULL arrays
        rig.model.store([], resets, horizon, idx)
        r_d = _dev(resets)
        L._check(lib.arl_seq_store(None, 0, 0, r_d.data_ptr(), 2, horizon, size, S, idx, None, rig.ring.data_ptr(),
                                   L.stream_ptr()), "arl_seq_store")
        rig.compare(("NULL arrays", size))


@pytest.mark.parametrize("n_state", [1, 2])
def test_seq_store_block_index_above_65535(L, n_state):
    rig = _SeqRig(70000, 2, 1, 4, n_state)
    rig.store(L, 1, 1)
    rig.store(L, 1, 0, flag=2)
    assert not np.isnan(rig.model.stores[0][69999]).any()


# ---- arl_seq_prepare -------------------------------------------------------------------------------------------------------

def _filled_rig(n_env, size, S, hidden, n_state):
    """a rig whose stores and ring hold random bits (the planted -0.0, denormal and inf included), put there by the host"""
    rig = _SeqRig(n_env, size, S, hidden, n_state)
    for st, dev in zip(rig.model.stores, rig.stores):
        st[...] = rig.rs.randn(*st.shape).astype(F32)
        st.reshape(-1)[:3] = np.array([-0.0, 1e-42, np.inf], F32)
        st[-1, -1, -1] = F32(-1e-42)                            # the last float of the last slot of the last environment
        dev.copy_(_dev(st))
    rig.model.ring[...] = rig.rs.randint(0, 200, size=rig.model.ring.shape).astype(np.uint8)
    rig.ring.copy_(_dev(rig.model.ring))
    return rig


def _prepare_and_compare(L, rig, env, slot, U, raw_null=False):
    env, slot = np.asarray(env, np.int32), np.asarray(slot, np.int32)
    b = len(env)
    er_big, env_rows = _guarded((b * U,), fill=-7, dtype=torch.int32)
    sr_big, step_rows = _guarded((b * U,), fill=-7, dtype=torch.int32)
    ro_big, r_out = _guarded((b * U,), fill=99, dtype=torch.uint8)
    made = [_guarded((b, rig.hidden)) for _ in range(rig.n_state)]
    env_d, slot_d = _dev(env), _dev(slot)
    if raw_null:
        assert rig.n_state == 0
        L._check(L.load().arl_seq_prepare(env_d.data_ptr(), slot_d.data_ptr(), b, U, rig.size, rig.S, None, 0, 0,
                                          rig.ring.data_ptr(), env_rows.data_ptr(), step_rows.data_ptr(), None,
                                          r_out.data_ptr(), L.stream_ptr()), "arl_seq_prepare")
    else:
        L.seq_prepare(env_d, slot_d, U, rig.size, rig.S, rig.stores, rig.ring, env_rows, step_rows, [m[1] for m in made],
                      r_out)
    torch.cuda.synchronize()
    w_env, w_step, w_states, w_resets = rig.model.prepare(env, slot, U)
    what = (rig.size, rig.S, rig.hidden, rig.n_state, U, b)
    np.testing.assert_array_equal(_host(env_rows), w_env, err_msg=str(what))
    np.testing.assert_array_equal(_host(step_rows), w_step, err_msg=str(what))
    np.testing.assert_array_equal(_host(r_out), w_resets, err_msg=str(what))
    assert _tail_untouched(er_big, b * U, -7) and _tail_untouched(sr_big, b * U, -7) and _tail_untouched(ro_big, b * U, 99)
    for (big, got), want in zip(made, w_states):
        np.testing.assert_array_equal(_bits(_host(got)), _bits(want), err_msg=str(what))
        assert _tail_untouched(big, want.size), what
    rig.compare(("prepare reads only",) + what)                  # the stores and the ring are inputs
    return w_step


def _all_pairs(n_env, n_slots):
    """every slot of every environment, then repeats of the last slot of the last environment and of (0, 0)"""
    env = np.concatenate([np.repeat(np.arange(n_env), n_slots), [n_env - 1, n_env - 1, 0]])
    slot = np.concatenate([np.tile(np.arange(n_slots), n_env), [n_slots - 1, n_slots - 1, 0]])
    return env, slot


@pytest.mark.parametrize("n_state", [0, 1, 2])
def test_seq_prepare_second_trip_over_t_at_the_hidden_limit(L, n_state):
    """U = 600 on a ring of 1040: three trips over t, sequences from slot 110 on wrap; hidden = 1024: 256 float4."""
    rig = _filled_rig(2, 1040, 4, 1024 if n_state else 0, n_state)
    env, slot = _all_pairs(2, 260)
    steps = _prepare_and_compare(L, rig, env, slot, 600)
    assert (np.diff(steps.reshape(len(env), 600), axis=1) < 0).any() and env[-3] == 1 and slot[-3] == 259


@pytest.mark.parametrize("hidden,n_state", [(4, 1), (4, 2), (1024, 2), (0, 0)])
def test_seq_prepare_sequences_that_lap_the_ring_twice(L, hidden, n_state):
    rig = _filled_rig(3, 40, 8, hidden, n_state)
    env, slot = _all_pairs(3, 5)
    steps = _prepare_and_compare(L, rig, env, slot, 100, raw_null=(n_state == 0))
    laps = (np.diff(steps.reshape(len(env), 100), axis=1) < 0).sum(axis=1)
    assert laps.min() == 2 and laps.max() == 3                   # 100 steps from slot k * 8 pass index 39 twice or thrice


def test_seq_prepare_a_batch_of_70000_sequences_of_one_step(L):
    rig = _filled_rig(3, 40, 8, 4, 1)
    rs = np.random.RandomState(70000)
    env, slot = rs.randint(0, 3, size=70000), rs.randint(0, 5, size=70000)
    env[-1], slot[-1] = 2, 4                                     # block 69999 reads the last slot of the last environment
    _prepare_and_compare(L, rig, env, slot, 1)


# ---- arl_r2d2_loss ---------------------------------------------------------------------------------------------------------

NOT_BIT_EQUAL = dict(elements=0, differing=0)


def _loss_configs():
    """(eps, weighted, eta, gamma_n or None for the shape's own 0.997^n)"""
    out = [(eps, w, eta, None) for eps in (1e-3, 0.0) for w in (True, False) for eta in (0.0, 1.0, 0.9)]
    return out + [(1e-3, True, 0.9, 0.0)]


@pytest.mark.parametrize("shape", rr.LIMIT_SHAPES, ids=str)
def test_r2d2_loss_at_its_limits_within_one_ulp_of_float64(L, shape):
    batch, burn_in, train_len, n, n_act, stride, duel = shape
    U = burn_in + train_len + n
    own_gamma = 0.997 ** n
    c = rr.limits_loss_case(10 * batch + n_act, *shape, gamma_n=own_gamma)
    q, qt = c["q"], c["q_tgt"]
    first, last = burn_in, burn_in + train_len - 1
    assert c["terminals"][first] and c["terminals"][last] and c["actions"][batch * U - n - 1] == 255
    assert (q[:, n_act + duel:] == rr.PAD).all() and (qt[:, n_act + duel:] == rr.PAD).all()
    dc = {k: _dev(v) for k, v in c.items()}
    # exact +0 outside the train window, in the padding columns and (without dueling) in every other action
    zero = np.ones((batch, U, stride), bool)
    act = np.minimum(c["actions"].astype(np.int64), n_act - 1).reshape(batch, U)
    if duel:
        zero[:, burn_in:burn_in + train_len, :n_act + 1] = False
    else:
        bb, tt = np.meshgrid(np.arange(batch), np.arange(burn_in, burn_in + train_len), indexing="ij")
        zero[bb, tt, act[bb, tt]] = False
    differing_here = 0
    for eps, weighted, eta, g in _loss_configs():
        gamma_n = own_gamma if g is None else g
        want = rr.r2d2_loss64(q, qt, c["actions"], c["returns"], c["terminals"], c["is_weights"] if weighted else None,
                              batch, burn_in, train_len, n, n_act, bool(duel), gamma_n, eps, eta)
        assert (want["x"] == 0).any() and (want["z"] == 0).any() and want["a_star"][0, 0] == 0
        assert np.abs(want["d"][0]).argmax() == train_len - 1    # the largest |d| of sequence 0 is its last
        dq_big, dq = _guarded((batch * U, stride))
        td_big, td = _guarded((batch, train_len))
        lr_big, loss_rows = _guarded((batch,))
        pr_big, prio = _guarded((batch,))
        L.r2d2_loss(dc["q"], dc["q_tgt"], dc["actions"], dc["returns"], dc["terminals"],
                    dc["is_weights"] if weighted else None, batch, burn_in, train_len, n, n_act, gamma_n, eps, eta, dq, td,
                    loss_rows, prio, dueling=bool(duel))
        torch.cuda.synchronize()
        what = "%s eps %g weights %s eta %g gamma_n %g" % (shape, eps, weighted, eta, gamma_n)
        assert _tail_untouched(dq_big, batch * U * stride) and _tail_untouched(td_big, batch * train_len), what
        assert _tail_untouched(lr_big, batch) and _tail_untouched(pr_big, batch), what
        got = dict(dq=_host(dq), td_abs=_host(td), loss_rows=_host(loss_rows), priorities=_host(prio))
        for key in ("dq", "td_abs", "loss_rows", "priorities"):
            assert np.isfinite(got[key]).all(), (what, key)
            ok = rr.within_one_ulp(got[key], want[key])
            differing = int((_bits(got[key]) != _bits(want[key])).sum())
            NOT_BIT_EQUAL["elements"] += got[key].size
            NOT_BIT_EQUAL["differing"] += differing
            differing_here += differing
            if differing or not ok.all():
                print("%s %s: %d of %d elements not bit-equal, %d outside 1 ulp (bound: 0)" % (
                    what, key, differing, got[key].size, int((~ok).sum())))
            assert ok.all(), (what, key)
        assert (_bits(got["dq"]).reshape(batch, U, stride)[zero] == 0).all(), what
        assert (got["dq"].reshape(batch, U, stride)[~zero] != 0).any()
        # the priorities are the mix of the returned |d|'s maximum and mean
        t64 = got["td_abs"].astype(np.float64)
        s, mx = np.zeros(batch), np.zeros(batch)
        for t in range(train_len):
            s = s + t64[:, t]
            mx = np.maximum(mx, t64[:, t])
        again = (eta * mx + (1.0 - eta) * (s / float(train_len))).astype(np.float32)
        assert rr.within_one_ulp(got["priorities"], again).all(), what
        if train_len > 1:                                        # sequence 0's maximum is its last entry: eta = 1 returns it
            assert eta != 1.0 or got["priorities"][0] == got["td_abs"][0, -1], what
    for k, v in c.items():                                       # the inputs are inputs
        np.testing.assert_array_equal(_host(dc[k]), v)
    print("R2D2 limits %s: %d elements not bit-equal but within one ulp in this shape; so far %d of %d" % (
        shape, differing_here, NOT_BIT_EQUAL["differing"], NOT_BIT_EQUAL["elements"]))


# ---- arl_vmpo_weights ------------------------------------------------------------------------------------------------------

EPS_ETA = 0.01
PSI_NOT_BIT_EQUAL = dict(elements=0, differing=0)


def _run_weights(L, full_d, idx, duals, n_rows):
    psi_big, psi = _guarded((n_rows,))
    t_big, temp4 = _guarded((4,))
    L.vmpo_weights(full_d, idx, duals, EPS_ETA, psi, temp4)
    torch.cuda.synchronize()
    assert _tail_untouched(psi_big, n_rows) and _tail_untouched(t_big, 4)
    return _host(psi), _host(temp4)


def _check_weights(L, name, adv, eta, with_idx, rs):
    """arl_vmpo_weights on one set of advantages: the selection exact, psi within one ulp, temp4 within the ulp of the
    largest addend (where the float64 value is an fp32 number at all), two launches the same bits.  -> the temp4
    entries that were compared."""
    n = adv.size
    n_rows = 2 * n if with_idx else n
    rows = rs.permutation(n_rows)[:n].astype(np.int32) if with_idx else np.arange(n, dtype=np.int32)
    full = rs.randn(n_rows).astype(F32) * F32(50.)                  # (rows outside the minibatch: never read)
    full[rows] = adv
    idx = _dev(rows) if with_idx else None
    duals = torch.tensor([eta, 5.0], dtype=torch.float32, device=DEV)
    full_d = _dev(full)
    psi, temp4 = _run_weights(L, full_d, idx, duals, n_rows)
    ref = vr.weights(adv, eta, EPS_ETA)
    want = ref["psi"].astype(F32)
    got = psi[rows]
    outside = np.ones(n_rows, dtype=bool)
    outside[rows] = False
    assert np.isnan(psi[outside]).all(), name                        # rows outside the minibatch keep their fill
    assert (_bits(got[~ref["sel"]]) == 0).all(), name                # unselected rows are exactly +0
    if (want[ref["sel"]] > 0).all():
        assert np.array_equal(got > 0, ref["sel"]), name             # the selected set is the reference's
    else:
        assert name.startswith("near-flt-max"), name                 # the one family whose weights may underflow
        assert (got[want > 0] > 0).all(), name
    assert rr.within_one_ulp(got, want).all(), (name, np.abs(got - want).max())
    PSI_NOT_BIT_EQUAL["elements"] += n
    PSI_NOT_BIT_EQUAL["differing"] += int((_bits(got) != _bits(want)).sum())
    assert temp4[3] == ref["n_top"] == (n + 1) // 2
    compared = []
    for k, key in enumerate(("temp_loss", "d_eta", "L")):
        if not abs(ref[key]) <= FLT_MAX:
            continue
        ulp = np.spacing(F32(max(ref["addends"][k], abs(ref[key]))))
        assert np.isfinite(temp4[k]) and abs(float(temp4[k]) - ref[key]) <= ulp, (name, key, temp4[k], ref[key], ulp)
        compared.append(key)
    psi2, temp4_2 = _run_weights(L, full_d, idx, duals, n_rows)      # two launches give the same bits
    assert np.array_equal(_bits(psi), _bits(psi2)) and np.array_equal(_bits(temp4), _bits(temp4_2)), name
    return compared


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("n", vr.LIMIT_SIZES)
def test_vmpo_weights_with_each_radix_pass_and_bin_deciding(L, n, with_idx):
    rs = np.random.RandomState(7 * n + with_idx)
    for name, p, T, edge in vr.radix_families(n):
        k = vr.radix_case(np.random.RandomState(1000 * p + T + n), n, p, T, edge)    # the keys the host file examined
        trace, _, _ = vr.radix_trace(k)
        assert trace[p]["bin"] == T and (n == 1 or vr.first_deciding_pass(trace) == p), name
        adv = vr.from_keys(k)
        compared = _check_weights(L, name, adv, vr.eta_for(adv), with_idx, rs)
        assert compared == ["temp_loss", "d_eta", "L"], (name, compared)
    print("V-MPO radix cases n %d: psi so far %d of %d elements not bit-equal but within one ulp" % (
        n, PSI_NOT_BIT_EQUAL["differing"], PSI_NOT_BIT_EQUAL["elements"]))


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("n", vr.LIMIT_SIZES)
def test_vmpo_weights_across_the_sign_change_on_denormals_and_near_flt_max(L, n, with_idx):
    rs = np.random.RandomState(11 * n + with_idx)
    for name, adv, eta in vr.sign_and_range_cases(np.random.RandomState(n), n):
        compared = _check_weights(L, name, adv, eta, with_idx, rs)
        print("V-MPO %s n %d: temp4 entries compared: %s" % (name, n, ", ".join(compared) or "none"))
        assert name.startswith("near-flt-max") or compared == ["temp_loss", "d_eta", "L"], (name, compared)
    print("V-MPO sign / range cases n %d: psi so far %d of %d elements not bit-equal but within one ulp" % (
        n, PSI_NOT_BIT_EQUAL["differing"], PSI_NOT_BIT_EQUAL["elements"]))


# ---- SAC-Discrete ----------------------------------------------------------------------------------------------------------

def _guarded_launch_loss(c, gamma_n, delta_clip, log_alpha=None):
    """test_sacd_gpu._launch_loss with every output inside a larger NaN-filled buffer"""
    from accel_rl_amd import _lib
    q1 = _dev(c["q1"])
    batch, stride = q1.shape
    made = [_guarded((batch, stride)) for _ in range(3)]
    st_big, stats = _guarded((4, batch))
    la = torch.tensor([c["log_alpha"] if log_alpha is None else log_alpha, NAN, NAN, NAN], dtype=torch.float32, device=DEV)
    _lib.sacd_loss(q1, _dev(c["q2"]), _dev(c["t1"]), _dev(c["t2"]), _dev(c["lo"]), _dev(c["ln"]), _dev(c["act"]),
                   _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), la, c["n_act"], gamma_n, delta_clip, made[0][1],
                   made[1][1], made[2][1], stats)
    torch.cuda.synchronize()
    for big, _ in made:
        assert _tail_untouched(big, batch * stride)
    assert _tail_untouched(st_big, 4 * batch)
    return made[0][1].cpu(), made[1][1].cpu(), made[2][1].cpu(), stats.cpu()


@pytest.mark.parametrize("delta_clip", [None, 1.0], ids=["squared", "huber"])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("shape", sr.LIMIT_SHAPES, ids=lambda s: "A%d-S%d-B%d" % s[:3])
def test_sacd_loss_over_several_workgroups_and_at_the_action_limit(monkeypatch, shape, weighted, delta_clip):
    """test_sacd_gpu._check_loss -- sacd_ref.ref_loss and its per-element bounds, as they stand -- on guarded outputs."""
    monkeypatch.setattr(tsg, "_launch_loss", _guarded_launch_loss)
    c = sr.limit_case(shape, weighted)
    worst = tsg._check_loss(c, sr.GAMMA, delta_clip)
    print("SAC-D limits A%d S%d B%d %s %s: largest error / bound %.3f" % (
        shape[:3] + ("weighted" if weighted else "uniform", "huber" if delta_clip else "squared", worst)))
    again = _guarded_launch_loss(c, sr.GAMMA, delta_clip)           # two launches give the same bits
    for x, y in zip(again, _guarded_launch_loss(c, sr.GAMMA, delta_clip)):
        assert torch.equal(x, y)


def _launch_act(logits, n_act, override=None, deterministic=False):
    from accel_rl_amd import _lib
    batch = logits.shape[0]
    p_big, prob = _guarded((batch, n_act))
    g_big, greedy = _guarded((batch,), fill=255, dtype=torch.uint8)
    _lib.sacd_act(_dev(logits), _dev(override), n_act, prob, greedy, deterministic=deterministic)
    torch.cuda.synchronize()
    assert _tail_untouched(p_big, batch * n_act) and _tail_untouched(g_big, batch, 255)
    return prob.cpu().double().numpy(), greedy.cpu().numpy()


def test_sacd_act_at_the_action_limit_over_two_workgroups():
    n_act, stride, batch = 255, 256, 257
    c = sr.case(31 + n_act, n_act, stride, batch, False, shift=n_act)
    z = c["lo"]
    for row in (0, 256):                                        # a tie between action 0 and action 254: 0 is greedy
        z[row, :n_act] = -1.0
        z[row, 0] = z[row, 254] = 3.0
    z[1, :n_act] = -2.0
    z[1, 254] = 0.5                                             # the last action alone ahead
    assert (z[:, 255] == sr.POISON).all()
    want, greedy, atol = sr.ref_act(z, n_act)
    assert greedy[0] == greedy[256] == 0 and greedy[1] == 254
    got, g = _launch_act(z, n_act)
    assert np.isfinite(got).all() and (np.abs(got - want) <= atol).all()
    print("act limits A%d B%d: largest soft-max error / bound %.3f" % (n_act, batch, (np.abs(got - want) / atol).max()))
    assert (np.abs(got.sum(axis=1) - 1.0) <= 4 * 2.0 ** -23 * n_act).all()
    assert (g == greedy).all()
    got_d, g_d = _launch_act(z, n_act, deterministic=True)
    assert (g_d == greedy).all() and (got_d == np.eye(n_act)[greedy]).all()
    rs = np.random.RandomState(n_act)
    ov = np.where(rs.rand(batch) < 0.5, rs.randint(0, n_act, size=batch), -1).astype(np.int32)
    ov[0], ov[256], ov[2] = 254, 254, -1                         # the last action forced in both workgroups
    for det in (False, True):
        want_o, _, _ = sr.ref_act(z, n_act, override=ov, deterministic=det)
        got_o, g_o = _launch_act(z, n_act, override=ov, deterministic=det)
        forced = ov >= 0
        assert (got_o[forced] == want_o[forced]).all() and (g_o == greedy).all()
        assert got_o[0, 254] == 1 and got_o[256, 254] == 1 and got_o[0].sum() == 1 and got_o[256].sum() == 1
        assert (got_o[~forced] == (got_d if det else got)[~forced]).all()


@pytest.mark.parametrize("batch", sr.ALPHA_GRAD_BATCHES)
def test_sacd_alpha_grad_bit_for_bit_in_the_stated_order(batch):
    """log_alpha = 0: expf(0) is exactly 1, and entry 0 is the fp32 restatement of the header's order, bit for bit
    (the host half shows that a plain ascending sum, or the fold without its last step, gives other bits)."""
    from accel_rl_amd import _lib
    ent = sr.alpha_grad_rows(batch)
    want = sr.alpha_grad32(ent, sr.ALPHA_GRAD_TARGET)
    la = torch.tensor([0.0, NAN, NAN, NAN], dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):
        big, out = _guarded((4,))
        _lib.sacd_alpha_grad(_dev(ent), la, float(sr.ALPHA_GRAD_TARGET), out)
        torch.cuda.synchronize()
        assert _tail_untouched(big, 4)
        outs.append(_host(out))
    got = outs[0]
    print("alpha grad B %d: got %.9g want %.9g" % (batch, got[0], want))
    assert _bits(got[:1])[0] == _bits(np.array([want]))[0], (got[0], want)
    assert (_bits(got[1:]) == 0).all()                           # entries 1 .. 3 are +0
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    ref, atol = sr.ref_alpha_grad(ent, np.float32(0.0), float(sr.ALPHA_GRAD_TARGET))
    assert abs(float(got[0]) - ref) <= atol
