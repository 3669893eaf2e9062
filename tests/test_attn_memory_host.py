"""AtariAttnMemoryPolicy without a device: the constructor's refusals, the state keys, the parameter layout and
tattn_shape_ok."""
import pytest

TRUNK = dict(conv_filters=(8, 8), conv_filter_sizes=(4, 3), conv_strides=(2, 1), conv_pads=((0, 0), (0, 0)))


def _policy(**kw):
    from accel_rl_amd.policies import AtariAttnMemoryPolicy
    return AtariAttnMemoryPolicy(**dict(dict(TRUNK, hidden_sizes=(16,), memory_len=4, n_heads=2, head_dim=8), **kw))


@pytest.mark.parametrize("change", [dict(hidden_sizes=()), dict(hidden_sizes=(16, 16)), dict(hidden_sizes=(18,)),
                                    dict(memory_len=0), dict(memory_len=65), dict(memory_len=2.0), dict(head_dim=6),
                                    dict(head_dim=68), dict(n_heads=0), dict(n_heads=5, head_dim=64),
                                    dict(hidden_sizes=(256,), memory_len=5)])
def test_constructor_refusals_name_the_section(change):
    from accel_rl_amd.policies import AtariAttnMemoryPolicy
    with pytest.raises(NotImplementedError, match="section E"):
        AtariAttnMemoryPolicy(**dict(dict(TRUNK, hidden_sizes=(16,), memory_len=4, n_heads=2, head_dim=8), **change))


def test_state_keys_and_layout():
    p = _policy()
    assert p.recurrent and p.state_info_keys == ["mem_0"] and p.supports_bptt_resets and not p.serve_supported()
    layout = p.reference_layout((4, 20, 16), 5)
    assert [n for n, _ in layout][4:11] == ["AttnWx", "AttnBx", "AttnWq", "AttnWkv", "AttnWo", "AttnBo", "AttnRel"]
    assert dict(layout[4:11]) == dict(AttnWx=(8 * 7 * 5, 16), AttnBx=(16,), AttnWq=(16, 16), AttnWkv=(16, 32),
                                      AttnWo=(16, 16), AttnBo=(16,), AttnRel=(2, 5))
    assert _policy(hidden_sizes=(256,), memory_len=4, n_heads=4, head_dim=64).reference_layout((4, 104, 80), 6)[-1] == (
        "Outputb", (1,))


def test_tattn_shape_ok():
    from accel_rl_amd import _lib
    ok = _lib.tattn_shape_ok
    assert ok(1, 1, 1, 4) and ok(64, 64, 4, 64) and ok(20, 16, 2, 32)
    assert not any((ok(0, 1, 1, 4), ok(65, 1, 1, 4), ok(1, 0, 1, 4), ok(1, 65, 1, 4), ok(1, 1, 0, 4), ok(1, 1, 1, 6),
                    ok(1, 1, 1, 68), ok(1, 1, 5, 64)))
