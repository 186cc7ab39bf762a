"""The numpy restatement of the DG-SIP operator with Neumann faces (tests/dg_mixed_reference.py) on the CPU: the
properties that make a boundary face without a contribution to the form a Neumann face, the dense solves the GPU test
reproduces, and the host helper that marks the sides of a box.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import dg_oracle as dg

import dg_mixed_reference as mx
import dg_reference_2d as ref2

KINDS = [dg.HERMITE, dg.GAUSS_LOBATTO, dg.GAUSS]
KIND_IDS = ["hermite", "gl", "gauss"]
SHEARED_2D = np.array([[1.12, 0.24], [0.24, 1.48]]) @ np.diag([0.95, 0.89])
SHEARED_3D = dg.cheby_mesh(2)[1]


def sheared_box(dim, p, kind, sides, cells=None):
    if dim == 3:
        return mx.mixed_oracle(p, kind, cells or (2, 1, 2), SHEARED_3D, sides)
    return mx.mixed_oracle(p, kind, cells or (3, 2), SHEARED_2D, sides)


def polynomial(dim, p):
    """u = (1 + a.x)^p, total degree p, -Laplace u and grad u"""
    a = np.array([0.3, -0.2, 0.5][:dim])
    u = lambda x: (1.0 + x @ a) ** p                                               # noqa: E731
    f = lambda x: -p * (p - 1) * (a @ a) * (1.0 + x @ a) ** max(p - 2, 0)          # noqa: E731
    grad = lambda x: (p * (1.0 + x @ a) ** (p - 1))[..., None] * a                  # noqa: E731
    return u, f, grad


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_symmetric_and_definite_with_one_dirichlet_side(dim, kind):
    """every side but one Neumann: symmetric to rounding, and positive definite"""
    o = sheared_box(dim, 2, kind, range(1, 2 * dim))
    A = mx.MixedRhsReference(o).dense_matrix()
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
    ev = np.linalg.eigvalsh(0.5 * (A + A.T))
    assert ev[0] > 1e-6 * ev[-1]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_all_neumann_box_has_the_constants_as_null_space(dim, kind):
    o = sheared_box(dim, 2, kind, range(2 * dim))
    A = mx.MixedRhsReference(o).dense_matrix()
    one = mx.MixedRhsReference(o).interpolate(lambda x: np.ones(x.shape[:-1])).ravel()
    assert abs(A @ one).max() <= 1e-13 * abs(A).max()
    assert abs(o.vmult(one)).max() <= 1e-13 * abs(A).max()
    ev = np.linalg.eigvalsh(0.5 * (A + A.T))
    assert abs(ev[0]) <= 1e-12 * ev[-1] and ev[1] > 1e-6 * ev[-1]       # exactly one


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dim", [2, 3])
def test_polynomial_identity(dim, p, kind):
    """A interpolate(u) = load(-Laplace u) + dirichlet_load(u) + neumann_load(d_n u) for a polynomial of total degree
    <= p on a sheared box: integration by parts leaves int_F d_n u phi_i on a face that contributes nothing to the form"""
    sides = (0, 3) if dim == 2 else (1, 2, 4)
    o = sheared_box(dim, p, kind, sides)
    r = mx.MixedRhsReference(o, origin=[-0.9, 0.3, 0.1][:dim])
    u, f, grad = polynomial(dim, p)
    lhs = o.vmult(r.interpolate(u))
    rhs = r.load_vector(f) + r.boundary_load(u) + r.neumann_load(grad)
    assert abs(lhs - rhs).max() < 1e-12 * abs(rhs).max()
    # the sampled flux is what neumann_load integrates
    flux = r.sample_flux(grad)
    again = np.zeros(o.shape)
    for pos in r.cell_positions():
        for face in r.neumann_faces(pos):
            again[r._at(pos)] += r.trace[face].T @ (r.face[face][1] * flux[r._at(pos)][face])
    assert abs(again - r.neumann_load(grad)).max() <= 1e-14 * abs(again).max()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dim", [2, 3])
def test_transformed_diagonal_is_positive_but_for_the_all_neumann_cell(dim, p, kind):
    """diag(T^T A_KK T) for all 3^(2 dim) combinations of face kinds on a sheared cell.  The cell whose faces are all
    Neumann faces is the one whose block is singular (the constants); its transformed diagonal vanishes for the constant
    at p = 1 only (T does not hold the constant as a column otherwise), so the block itself is looked at."""
    o = (dg.DGOracle(p, kind, (1, 1, 1), SHEARED_3D) if dim == 3 else ref2.DGOracle2D(p, kind, (1, 1), SHEARED_2D))
    for kinds in mx.all_kind_combinations(dim):
        d = mx.transformed_diagonal(o, kinds)
        ev = np.linalg.eigvalsh(mx.own_block_of_kinds(o, kinds))
        if all(k == mx.NEUMANN for k in kinds):
            assert abs(ev[0]) <= 1e-12 * ev[-1] and ev[1] > 1e-6 * ev[-1]
            assert d.min() >= -1e-12 * d.max()
        else:
            assert d.min() > 1e-6 * d.max(), kinds
            assert ev[0] > 1e-8 * ev[-1], kinds


def test_dense_solves_with_two_neumann_sides_converge():
    """prod sin(3 pi x_d) on [-0.9, 1]^2, Hermite-like basis, p = 3, lower-x and upper-y sides Neumann with the exact
    flux, dense solves on 4^2, 8^2 and 16^2 cells: 3.009e-2, 3.041e-3, 2.608e-4, ratios 9.9 and 11.7 >= 2^p"""
    u = lambda x: np.prod(np.sin(3 * np.pi * x), axis=-1)                           # noqa: E731
    f = lambda x: 2 * (3 * np.pi) ** 2 * u(x)                                       # noqa: E731

    def grad(x):
        s, c = np.sin(3 * np.pi * x), 3 * np.pi * np.cos(3 * np.pi * x)
        return np.stack([c[..., 0] * s[..., 1], s[..., 0] * c[..., 1]], axis=-1)

    err = []
    for n in (4, 8, 16):
        o = mx.mixed_oracle(3, dg.HERMITE, (n, n), np.eye(2) * 1.9 / n, mx.DENSE_NEUMANN_SIDES_2D)
        r = mx.MixedRhsReference(o, origin=[-0.9, -0.9])
        b = r.load_vector(f) + r.boundary_load(u) + r.neumann_load(grad)
        err.append(r.l2_error(np.linalg.solve(r.dense_matrix(), b.ravel()), u))
    print("two Neumann sides", err)
    assert np.allclose(err, mx.DENSE_ERRORS_MIXED_2D_P3, rtol=1e-6)
    assert err[0] / err[1] >= 8 and err[1] / err[2] >= 8


@pytest.mark.parametrize("ordering", ["z", "lex"])
@pytest.mark.parametrize("cells,sides", [((3, 2), (0, 3)), ((1, 4), (0, 1, 2)), ((3, 1, 2), (0, 3, 4, 5)), ((2, 2, 2), ())])
def test_box_set_sides_against_numpy_marking(cells, sides, ordering):
    """mgx_dg_box_set_sides (host only): the boundary entries of the marked sides become -2, the others stay"""
    import multigrid_amd as mg
    plain_nb, pos = mg.dg_box_neighbours(cells, ordering)
    nb, pos2 = mg.dg_box_neighbours(cells, ordering, neumann_sides=sides)
    assert (pos == pos2).all()
    kinds = mx.neighbour_kinds(cells, sides, pos)
    assert (nb[kinds < 0] == kinds[kinds < 0]).all()
    assert (nb[kinds == 0] == plain_nb[kinds == 0]).all() and (plain_nb[kinds == 0] >= 0).all()
    assert (nb == mg.dg_box_set_sides(cells, pos, plain_nb.copy(), sides)).all()


def test_box_set_sides_refuses_what_does_not_fit():
    import multigrid_amd as mg
    from multigrid_amd import _lib
    lib = _lib.load()
    cells = (2, 3)
    nb, pos = mg.dg_box_neighbours(cells)
    i32p = C.POINTER(C.c_int32)

    def call(dim, cells, pos, kinds, table):
        return lib.mgx_dg_box_set_sides(dim, (C.c_int * len(cells))(*cells), pos.shape[0], pos.ctypes.data_as(i32p),
                                        (C.c_int * len(kinds))(*kinds), table.ctypes.data_as(i32p))

    before = nb.copy()
    assert call(2, cells, pos, [-1, -2, -1, -3], nb) == -1          # a kind that is neither
    assert call(4, cells, pos, [-1, -2, -1, -2], nb) == -1          # no such dimension
    assert call(2, (3, 3), pos, [-1, -2, -1, -2], nb) == -1         # another box: a boundary entry inside it
    assert b"mgx_dg_box_set_sides" in lib.mgx_last_error()
    shifted = np.ascontiguousarray(pos + 1)
    assert call(2, cells, shifted, [-1, -2, -1, -2], nb) == -1      # positions outside the box
    assert (nb == before).all()                                      # ... and the table is left alone
    assert call(2, cells, pos, [-1, -2, -1, -2], nb) == 0
