"""The host side of the degree transfer and its numpy reference, without a GPU: mgx_dg_degree_embedding (libmgx.so, host
only) against tests/dg_hp_reference.py::degree_embedding_1d for every pair of degrees and basis; properties that pin the
reference independently of the code under test; DGHPOracle on an h-only hierarchy against DGPlainOracle; and the
convergence of the reference on the hierarchies tests/test_gpu_dg_hp.py runs on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import dg_oracle as dg

import dg_hp_reference as hp
import dg_plain_reference as plain
import dg_reference_2d as ref2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(pf, pc) for pf in range(2, 10) for pc in range(1, pf)]
KINDS = (dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "multigrid_amd", "libmgx.so")):
        g.build()
    from multigrid_amd import _lib
    return _lib.load()


def host_embedding(lib, pf, pc, kind):
    E = np.full((pf + 1, pc + 1), np.nan)
    status = lib.mgx_dg_degree_embedding(pf, pc, kind, E.ctypes.data_as(C.POINTER(C.c_double)))
    return status, E


def test_host_embedding_matches_the_reference_for_every_pair_and_basis(lib):
    """1e-13: the tolerance test_gpu_dg_plain.py::test_transfer_matrix has for the h embedding"""
    assert len(PAIRS) == 36
    worst = {}
    for kind in KINDS:
        for pf, pc in PAIRS:
            status, E = host_embedding(lib, pf, pc, kind)
            assert status == 0
            worst[(kind, pf, pc)] = abs(E - hp.degree_embedding_1d(pf, pc, kind)).max()
    key = max(worst, key=worst.get)
    print("largest difference %.3e at (basis, pf, pc) = %r" % (worst[key], key))
    assert worst[key] < 1e-13


@pytest.mark.parametrize("pf,pc,kind,status", [(3, 3, 0, -1), (2, 4, 1, -1), (3, 0, 0, -4), (10, 2, 2, -4), (0, 0, 0, -4),
                                               (4, 2, 3, -4), (4, 2, -1, -4)])
def test_host_embedding_refuses_invalid_input(lib, pf, pc, kind, status):
    """-1: MGX_ERR_INVALID_ARGUMENT (pc >= pf), -4: MGX_ERR_UNSUPPORTED (a degree outside 1 .. 9, an unknown basis)"""
    E = np.full((11, 11), np.nan)
    assert lib.mgx_dg_degree_embedding(pf, pc, kind, E.ctypes.data_as(C.POINTER(C.c_double))) == status
    assert np.isnan(E).all()
    assert b"mgx_dg_degree_embedding" in lib.mgx_last_error()
    assert lib.mgx_dg_degree_embedding(3, 1, 0, None) == -1


# ---------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("kind", KINDS)
def test_a_coarse_function_and_its_prolongation_take_the_same_values(kind):
    rng = np.random.default_rng(1)
    x = rng.random(40)
    for pf, pc in PAIRS:
        fine, coarse = dg.basis_1d(pf, kind), dg.basis_1d(pc, kind)
        c = rng.standard_normal(pc + 1)
        f = hp.degree_embedding_1d(pf, pc, kind) @ c
        vc = sum(cj * phi(x) for cj, phi in zip(c, coarse))
        vf = sum(fi * phi(x) for fi, phi in zip(f, fine))
        assert abs(vf - vc).max() < 1e-12 * max(1.0, abs(vc).max()), (pf, pc)


@pytest.mark.parametrize("kind", KINDS)
def test_embeddings_compose(kind):
    for p3 in range(3, 10):
        for p2 in range(2, p3):
            for p1 in range(1, p2):
                E13 = hp.degree_embedding_1d(p3, p1, kind)
                E = hp.degree_embedding_1d(p3, p2, kind) @ hp.degree_embedding_1d(p2, p1, kind)
                assert abs(E - E13).max() < 1e-12 * max(1.0, abs(E13).max()), (p1, p2, p3)


@pytest.mark.parametrize("name", ["3d-p", "3d-ph-sheared", "2d-hp"])
def test_restriction_is_the_transpose_of_prolongation(name):
    kind, cells, hierarchy, jac = hp.SOLVER_CASES[name]
    o = hp.solved_case(name)["o"]
    rng = np.random.default_rng(2)
    for l in range(1, o.n_levels):
        c, f = rng.standard_normal(o.level[l - 1].shape), rng.standard_normal(o.level[l].shape)
        assert np.vdot(o.prolongate(l, c), f) == pytest.approx(np.vdot(c, o.restrict(l, f)), rel=1e-12)


def test_2d_oracle_is_both():
    o = hp.solved_case("2d-hp")["o"]
    assert isinstance(o, hp.DGHPOracle) and isinstance(o, ref2.DGPlainOracle2D)
    assert isinstance(hp.solved_case("3d-p")["o"], plain.DGPlainOracle)


@pytest.mark.parametrize("dim", [3, 2])
def test_h_only_hierarchy_is_the_plain_oracle(dim):
    if dim == 3:
        args = (2, dg.HERMITE, (2, 1, 1), hp.SHEARED_3D, 3)
        a = plain.DGPlainOracle(*args)
    else:
        args = (3, dg.GAUSS_LOBATTO, (2, 1), hp.SHEARED_2D, 3)
        a = ref2.DGPlainOracle2D(*args)
    p, kind, cells, jac, levels = args
    b = hp.DGHPOracle(kind, [(p, l) for l in range(levels)], cells, jac)
    assert a.info == b.info
    rng = np.random.default_rng(3)
    x = rng.standard_normal(a.level[-1].shape)
    assert np.array_equal(a.v_cycle(x), b.v_cycle(x))
    (xa, ia, ra), (xb, ib, rb) = a.solve_cg(x, 1e-9), b.solve_cg(x, 1e-9)
    assert np.array_equal(xa, xb) and ia == ib and ra == rb


@pytest.mark.parametrize("name", sorted(hp.SOLVER_CASES))
def test_reference_converges_on_the_gpu_cases(name):
    """the solver stops at 100 CG iterations; the reference takes 16 to 29 on these right-hand sides"""
    R = hp.solved_case(name)
    x, its, red = R["cg"]
    o = R["o"]
    print(name, "iterations", its, "reduction", red, [i["degree"] for i in o.info], [i["cg_its"] for i in o.info])
    assert its < 100
    assert np.linalg.norm(R["rhs"] - o.level[-1].vmult(x)) <= 1e-9 * np.linalg.norm(R["rhs"])


def test_reference_converges_with_a_neumann_side():
    R = hp.solved_case(hp.NEUMANN_CASE, hp.NEUMANN_SIDES)
    x, its, red = R["cg"]
    print("iterations", its, "reduction", red)
    assert its < 100
    assert np.linalg.norm(R["rhs"] - R["o"].level[-1].vmult(x)) <= 1e-9 * np.linalg.norm(R["rhs"])
