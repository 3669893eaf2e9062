"""NGU's episodic bonus without a GPU: the constructors' refusals, the new entry points in the binding table and the
built library, and tests/ngu_ref.py on an example computed by hand."""
import numpy as np
import pytest

import ngu_ref

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("kwargs,match", [
    (dict(memory_size=0), "memory_size"), (dict(memory_size=4097), "memory_size"), (dict(memory_size=8.0), "memory_size"),
    (dict(k=0), "k must"), (dict(k=17), "k must"), (dict(eps=0.), "eps"), (dict(eps=float("nan")), "eps"),
    (dict(c=-1e-3), "c:"), (dict(xi=float("inf")), "xi"), (dict(s_max=0.), "s_max"), (dict(mod_clip=0.5), "mod_clip"),
    (dict(ngu_args=dict(width=32)), "unknown keys"), (dict(ngu_args=dict(embedding_size=132)), "embedding_size"),
    (dict(ngu_args=dict(embedding_size=30)), "embedding_size"), (dict(ngu_args=dict(seed=-1)), "seed"),
    (dict(ngu_args=dict(head_hidden=260)), "head_hidden"), (dict(ngu_args=dict(embedding_size=128)), "head_hidden"),
    (dict(int_coeff=float("nan")), "int_coeff")], ids=lambda v: str(v) if isinstance(v, str) else None)
def test_constructor_refusals(kwargs, match):
    from accel_rl_amd.algos.pg import NguA2C, NguPPO
    for cls in (NguPPO, NguA2C):
        with pytest.raises(ValueError, match=match):
            cls(**kwargs)
    with pytest.raises(ValueError, match="update_proportion must be 1"):
        NguA2C(update_proportion=0.5)


def test_the_entry_points_are_bound_and_exported():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    assert lib.arl_abi_version() == 5
    assert {"arl_epi_knn", "arl_epi_mix", "arl_invdyn_loss_parts", "arl_invdyn_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.arl_invdyn_workspace_bytes(32, 128, 18) == 64 * 4 * (64 * 128 + 128 + 128 * 18 + 20 + 4)
    assert lib.arl_invdyn_workspace_bytes(128, 68, 18) == 0
    assert lib.arl_invdyn_loss_parts(*[None] * 7, 1, 4, 4, 2, *[None] * 9) == -1
    # argument errors come back before any HIP call
    assert lib.arl_epi_knn(None, None, 1, 1, 4, 1, 1, None, None, None, None, None) == -1
    assert lib.arl_epi_mix(None, None, None, None, 1, 1, None, None, 1e-3, 1e-3, 8e-3, 8., 5., 1., 1., None, None, None) == -1
    assert b"null" in lib.arl_last_error()


def test_restatement_on_three_rows_by_hand():
    """One env, M = 2, k = 2, E = 4, embeddings (0,0,0,0), (3,4,0,0), (3,4,0,0), then a second rollout of one done row."""
    emb = np.array([[[0, 0, 0, 0], [3, 4, 0, 0], [3, 4, 0, 0]]], F32)
    knn, m, mem, n_ins = ngu_ref.knn(emb, np.zeros((1, 3), np.uint8), np.zeros((1, 2, 4), F32), np.zeros(1, np.int32), 2)
    assert m.tolist() == [0, 1, 2] and n_ins.tolist() == [3]
    assert knn.tolist() == [[np.inf, np.inf], [25.0, np.inf], [0.0, 25.0]]
    assert mem[0].tolist() == [[3, 4, 0, 0], [3, 4, 0, 0]]              # entry 2 overwrote entry 0 in slot 0
    # the mix: the mean distance is 50 / 3; row 2: dn = (0, 1.5 - xi) -> K = (1, eps / (1.5 - xi + eps))
    eps, c, xi = 1e-3, 1e-3, 8e-3
    r_mix, dist, mom, diag = ngu_ref.mix(knn, m, None, np.array([1, 1, -1], F32), np.zeros(2), np.zeros(3), eps, c, xi, 8.,
                                         5., 1., 2.)
    assert dist.tolist() == [3.0, 50.0 / 3.0] and mom.tolist() == [0, 0, 0]
    r1 = 1.0 / (np.sqrt(eps / (1.5 - xi + eps)) + c)
    r2 = 1.0 / (np.sqrt(1.0 + eps / (1.5 - xi + eps)) + c)
    assert r1 > r2 > 1 / 8.                                                 # (the first visit pays more; both below s_max)
    assert np.allclose(r_mix, [1.0, 1.0 + 2 * r1, -1.0 + 2 * r2], rtol=1e-6)
    assert np.allclose(diag, [(r1 + r2) / 3, 1.0, 50.0 / 3.0], rtol=1e-6)
    # s_max below the revisit's similarity: its bonus is 0
    assert ngu_ref.mix(knn, m, None, np.zeros(3, F32), np.zeros(2), np.zeros(3), eps, c, xi, 1.0, 5., 1., 2.)[0][2] == 0
    # a done row: no neighbours, the ring cleared, the row itself entry 0
    knn, m, mem, n_ins = ngu_ref.knn(np.ones((1, 1, 4), F32), np.ones((1, 1), np.uint8), mem, n_ins, 2)
    assert m.tolist() == [0] and n_ins.tolist() == [1] and mem[0].tolist() == [[1, 1, 1, 1], [0, 0, 0, 0]]
