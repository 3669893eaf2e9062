"""CPU-only: the host side of reset-aware BPTT.  The header, the binding and the built library agree on
the four new entry points, they report argument errors without a device, and AdvActorCriticBase.initialize lets a
recurrent policy through under mid_batch_reset=True only with bptt_resets=True and a policy that takes the flags."""
import ctypes
import os
import re
import types

import pytest

from conftest import ROOT

NEW = ("arl_seq_handover", "arl_lstm_cell_bwd_reset", "arl_gru_cell_bwd_reset", "arl_rnn_cell_bwd_reset")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def test_header_binding_and_library_agree_on_the_new_names(lib):
    from accel_rl_amd import _lib
    text = open(os.path.join(ROOT, "include", "accel_rl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(arl_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(os.path.join(ROOT, "accel_rl_amd", "libaccel_rl_hip.so"))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert getattr(raw, name) is not None
    for wrapper in ("seq_handover", "lstm_cell_bwd_reset", "gru_cell_bwd_reset", "rnn_cell_bwd_reset"):
        assert callable(getattr(_lib, wrapper))
    assert lib.arl_abi_version() == 5 == _lib.ARL_ABI_VERSION


def test_new_entry_points_report_argument_errors_without_a_device(lib):
    # host memory stands in for the device pointers: every call below returns before anything is launched
    mem = (ctypes.c_char * 256)()
    p = ctypes.addressof(mem) + (-ctypes.addressof(mem)) % 16

    def handover(h_prev=p, h_stride=8, c_prev=p, c_stride=8, reset=p, idx=None, row0=0, step=5, batch=2, hidden=8, hp=p,
                 hprev_out=p, hprev_stride=8, cprev_out=p, cprev_out_stride=8):
        return lib.arl_seq_handover(h_prev, h_stride, c_prev, c_stride, reset, idx, row0, step, batch, hidden, hp,
                                    hprev_out, hprev_stride, cprev_out, cprev_out_stride, None)
    for kw in (dict(h_prev=None), dict(reset=None), dict(hp=None), dict(hprev_out=None), dict(c_prev=None),
               dict(cprev_out=None)):
        assert handover(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(hidden=6), dict(hidden=1028), dict(hidden=0), dict(batch=0), dict(batch=(1 << 24) + 1),
               dict(h_stride=4), dict(hprev_stride=(1 << 28) + 4), dict(cprev_out_stride=0), dict(row0=-1), dict(step=0),
               dict(row0=2 ** 31 - 1), dict(step=2 ** 31)):
        assert handover(**kw) == E_RANGE, kw
        assert b"arl_seq_handover" in lib.arl_last_error()
    for kw in (dict(h_prev=p + 4), dict(hp=p + 8), dict(hprev_out=p + 4), dict(c_stride=10), dict(hprev_stride=9)):
        assert handover(**kw) == E_ALIGN, kw

    def lstm(reset=p, row0=0, step=5, gates=p, batch=2, dg_stride=32):
        return lib.arl_lstm_cell_bwd_reset(p, 8, p, p, gates, 32, p, 8, p, 8, batch, 8, p, dg_stride, p, reset, None, row0,
                                           step, None)

    def gru(reset=p, row0=0, step=5, saved=p, batch=2, dgh_stride=24):
        return lib.arl_gru_cell_bwd_reset(p, 8, p, p, saved, 32, p, 8, batch, 8, p, 24, p, dgh_stride, p, reset, None, row0,
                                          step, None)

    def rnn(reset=p, row0=0, step=5, h=p, batch=2, d_stride=8):
        return lib.arl_rnn_cell_bwd_reset(p, 8, p, h, 8, batch, 8, p, d_stride, reset, None, row0, step, None)
    for fn, name, null, stride in ((lstm, b"arl_lstm_cell_bwd_reset", dict(gates=None), dict(dg_stride=31)),
                                   (gru, b"arl_gru_cell_bwd_reset", dict(saved=None), dict(dgh_stride=(1 << 28) + 1)),
                                   (rnn, b"arl_rnn_cell_bwd_reset", dict(h=None), dict(d_stride=7))):
        assert fn(**null) == E_ARG and name in lib.arl_last_error()
        for kw in (stride, dict(batch=0), dict(row0=-1), dict(step=0), dict(row0=2 ** 31 - 5, step=5)):
            assert fn(**kw) == E_RANGE and name in lib.arl_last_error(), (name, kw)
        assert fn(reset=None, **stride) == E_RANGE          # the checks do not depend on the flags being there


class _Recurrent:
    recurrent = True
    supports_bptt_resets = True
    state_info_keys = ["hprev_0", "cprev_0"]
    device = "cpu"
    distribution = types.SimpleNamespace(dist_info_keys=["prob"])

    def loss_and_grads(self, *a, **k):
        raise AssertionError("not reached")


class _RecurrentWithoutSupport(_Recurrent):
    supports_bptt_resets = False


class _RecurrentNeverHeardOfIt:
    recurrent = True
    state_info_keys = ["hprev_0"]
    device = "cpu"
    distribution = types.SimpleNamespace(dist_info_keys=["prob"])


class _Accepted(Exception):
    pass


def _algo(cls, **kw):
    """The algorithm with an optimizer that records what `initialize` hands it and stops there (the bucket set-up needs
    a device)."""
    algo = cls(**kw)
    seen = {}

    def initialize(inputs, **rest):
        seen["inputs"] = list(inputs)
        raise _Accepted
    algo.optimizer.initialize = initialize
    return algo, seen


def _algos():
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.ppo import RecurrentPPO
    return [(A2C, dict()), (RecurrentPPO, dict(optimizer_args=dict(minibatch_size=40)))]


def test_refused_by_default_with_a_message_that_names_the_flag():
    for cls, kw in _algos():
        algo, seen = _algo(cls, **kw)
        assert algo.bptt_resets is False
        with pytest.raises(NotImplementedError, match="bptt_resets=True"):
            algo.initialize(_Recurrent(), None, sample_size=80, horizon=5, mid_batch_reset=True)
        assert not seen


def test_accepted_with_the_flag_inputs_end_with_resets_and_hold_no_valids():
    for cls, kw in _algos():
        algo, seen = _algo(cls, bptt_resets=True, **kw)
        with pytest.raises(_Accepted):
            algo.initialize(_Recurrent(), None, sample_size=80, horizon=5, mid_batch_reset=True)
        names = seen["inputs"]
        assert names[-1] == "resets" and "valids" not in names and names.count("resets") == 1
        assert names[:5] == ["observations", "actions", "advantages", "returns", "old_value"]
        assert "hprev_0" in names and "cprev_0" in names
        assert algo._use_resets and not algo._use_valids


def test_the_flag_changes_nothing_without_mid_batch_reset_or_without_a_recurrent_policy():
    from accel_rl_amd.algos.pg.a2c import A2C
    feed_forward = types.SimpleNamespace(recurrent=False, state_info_keys=[], device="cpu",
                                         distribution=types.SimpleNamespace(dist_info_keys=["prob"]),
                                         loss_and_grads=None)
    got = {}
    for flag in (False, True):
        for what, policy, mbr in (("recurrent", _Recurrent(), False), ("ff", feed_forward, True), ("ff-", feed_forward, False)):
            algo, seen = _algo(A2C, bptt_resets=flag)
            with pytest.raises(_Accepted):
                algo.initialize(policy, None, sample_size=80, horizon=5, mid_batch_reset=mbr)
            got[flag, what] = seen["inputs"]
            assert "resets" not in seen["inputs"] and not algo._use_resets
            assert ("valids" in seen["inputs"]) == (not mbr)
    for what in ("recurrent", "ff", "ff-"):
        assert got[False, what] == got[True, what]


@pytest.mark.parametrize("policy_cls", [_RecurrentWithoutSupport, _RecurrentNeverHeardOfIt])
def test_a_policy_without_reset_support_is_refused_with_a_clear_message(policy_cls):
    for cls, kw in _algos():
        algo, seen = _algo(cls, bptt_resets=True, **kw)
        with pytest.raises(NotImplementedError, match="supports_bptt_resets") as e:
            algo.initialize(policy_cls(), None, sample_size=80, horizon=5, mid_batch_reset=True)
        assert policy_cls.__name__ in str(e.value) and not seen


def test_the_recurrent_policies_declare_support():
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_gru_policy import AtariGruPolicy
    from accel_rl_amd.policies.atari_lstm_policy import AtariLstmPolicy
    from accel_rl_amd.policies.atari_rnn_policy import AtariRnnPolicy
    for cls in (AtariLstmPolicy, AtariGruPolicy, AtariRnnPolicy):
        assert cls.supports_bptt_resets is True
    assert not getattr(AtariCnnPolicy, "supports_bptt_resets", False)
