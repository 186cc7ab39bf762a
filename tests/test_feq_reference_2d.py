"""The two-dimensional mesh provider (multigrid_amd.Square) against an independent enumeration, and the numpy reference
of tests/feq_reference_2d.py pinned to the 3D oracle through its 1D factors, checked for consistency and for the
discretisation error of its dense solve.  No GPU."""
import numpy as np
import pytest

import multigrid_amd as mg
from oracle import Oracle

import feq_reference_2d as ref

INVALID = 0xFFFFFFFF


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ---------------------------------------------------------------------------------------------
# provider
def local_dofs(idx9, p):
    """[n_cells, n, n] DoF of node (j, i) through the 9 entries of a cell, written out entity by entity"""
    n = p + 1
    out = np.empty((idx9.shape[0], n, n), dtype=np.int64)
    ix = idx9.astype(np.int64)
    for j in range(n):
        for i in range(n):
            cx, cy = (0 if i == 0 else 2 if i == p else 1), (0 if j == 0 else 2 if j == p else 1)
            if cx == 1 and cy == 1:
                off = (j - 1) * (p - 1) + (i - 1)
            elif cx == 1:
                off = i - 1
            elif cy == 1:
                off = j - 1
            else:
                off = 0
            out[:, j, i] = ix[:, 3 * cy + cx] + off
    return out


MESHES = [dict(n_subdiv=1, n_refine=1), dict(box=(3, 2), n_refine=2, h0=0.5, origin=-0.3)]


@pytest.mark.parametrize("mesh", range(len(MESHES)))
@pytest.mark.parametrize("p", range(1, 10))
def test_provider_tables(p, mesh):
    sq = mg.Square(p, **MESHES[mesh])
    n = p + 1
    for l in range(sq.n_levels):
        Nx, Ny = sq.cells_per_dim2(l)
        Gx, Gy = Nx * p + 1, Ny * p + 1
        cc = sq.cell_coords(l).astype(np.int64)
        assert sq.n_cells(l) == Nx * Ny == len(set(map(tuple, cc)))
        assert sq.n_dofs(l) == Gx * Gy
        # grid ids of every cell from its coordinates alone
        want = (cc[:, 1, None, None] * p + np.arange(n)[None, :, None]) * Gx + cc[:, 0, None, None] * p + np.arange(n)[None, None, :]
        plain, grid = sq.idx9_plain(l), sq.dof_grid(l).astype(np.int64)
        assert sorted(grid) == list(range(Gx * Gy))
        assert np.array_equal(grid[local_dofs(plain, p)], want)
        # contiguity: every entity is one block, the blocks tile [0, n_dofs)
        size = np.array([(p - 1 if e % 3 == 1 else 1) * (p - 1 if e // 3 == 1 else 1) for e in range(9)])
        blocks = {(int(b), int(s)) for row in plain for b, s in zip(row, size) if s}
        covered = np.zeros(sq.n_dofs(l), dtype=int)
        for b, s in blocks:
            covered[b:b + s] += 1
        assert (covered == 1).all()
        # constraints: exactly the boundary grid ids, numbered last; the constrained table is invalid there only
        gx, gy = grid % Gx, grid // Gx
        boundary = np.flatnonzero((gx == 0) | (gx == Gx - 1) | (gy == 0) | (gy == Gy - 1))
        con = sq.constrained(l)
        assert sorted(con) == list(boundary)
        assert sorted(con) == list(range(sq.n_dofs(l) - con.size, sq.n_dofs(l)))
        idx = sq.idx9(l)
        on_boundary = np.zeros(sq.n_dofs(l) + 1, dtype=bool)
        on_boundary[boundary] = True
        lattice_x, lattice_y = 2 * cc[:, 0, None] + np.arange(9)[None, :] % 3, 2 * cc[:, 1, None] + np.arange(9)[None, :] // 3
        edge = (lattice_x == 0) | (lattice_x == 2 * Nx) | (lattice_y == 0) | (lattice_y == 2 * Ny)
        assert np.array_equal(idx == INVALID, edge)
        assert np.array_equal(idx[~edge], plain[~edge])
        assert (plain != INVALID).all()
        has = size[None, :].repeat(len(plain), 0) > 0
        assert np.array_equal(on_boundary[plain[has]], edge[has])
        bi, bv = sq.bc(l)
        assert np.array_equal(bi, con)
        if l == 0:
            continue
        # children: quadrant c = x + 2y of the parent; weight_shift: log2 of the counted multiplicities
        ch, pc = sq.children(l), sq.cell_coords(l - 1).astype(np.int64)
        assert sorted(ch.ravel()) == list(range(sq.n_cells(l)))
        for c in range(4):
            assert np.array_equal(cc[ch[:, c]], 2 * pc + [c & 1, c >> 1])
        count = {}
        for prow in pc:
            for e in range(9):
                k = (4 * prow[0] + 2 * (e % 3), 4 * prow[1] + 2 * (e // 3))   # the patch entity on the fine entity lattice
                count[k] = count.get(k, 0) + 1
        ws = sq.weight_shift(l)
        for prow, wrow in zip(pc, ws):
            for e in range(9):
                assert 1 << int(wrow[e]) == count[(4 * prow[0] + 2 * (e % 3), 4 * prow[1] + 2 * (e // 3))]
    sq.close()


def test_provider_problem_data():
    """boundary values, right-hand side and L2 error of the provider against the reference's own quadrature"""
    for kw, A in ((dict(n_subdiv=2, n_refine=1), None), (dict(box=(3, 2), n_refine=1, h0=0.4, origin=-0.2, jacobian=[[1.0, 0.3], [0.1, 0.8]]),
                                                           [[1.0, 0.3], [0.1, 0.8]])):
        sq = mg.Square(3, **kw)
        e = ref.arrays_1d(sq)
        prob = ref.Problem(e, origin=kw.get("origin", -0.9), A=A)
        d = sq.operator_desc(1)
        assert d.dim == 2
        np.testing.assert_allclose(list(d.coef)[:3], prob.coef(), rtol=1e-14, atol=1e-15)
        L = ref.Level(e, sq.cells_per_dim2(1), prob.coef())
        g = sq.dof_grid(1)
        bi, bv = sq.bc(1)
        assert rel(bv, prob.boundary(L, sq.cell_size(1)).ravel()[g[bi]]) < 1e-13
        assert rel(sq.rhs(1), prob.rhs(L, sq.cell_size(1)).ravel()[g]) < 1e-12
        x = sq.seeded_vector(1, 5)
        xg = np.empty_like(x)
        xg[g] = x
        assert sq.l2_error(1, x) == pytest.approx(prob.l2_error(L, sq.cell_size(1), xg), rel=1e-12)
        cq = sq.coef_q(1)
        w = sq.qweights()
        np.testing.assert_allclose(cq[3], prob.coef()[:, None] * np.outer(w, w).ravel()[None, :], rtol=1e-14, atol=1e-16)
        sq.close()
    # the generator of the cube, keyed by the grid id
    sq, cube = mg.Square(2, 1, 1), mg.Cube(2, 1, 1)
    a, b = np.empty(sq.n_dofs(1)), np.empty(cube.n_dofs(1))
    a[sq.dof_grid(1)], b[cube.dof_grid(1)] = sq.seeded_vector(1, 9), cube.seeded_vector(1, 9)
    assert np.array_equal(a, b[:a.size])
    sq.close()
    cube.close()


# ---------------------------------------------------------------------------------------------
# reference against the 3D oracle through the 1D factors
@pytest.mark.parametrize("p", [1, 2, 4])
def test_kronecker_cube_of_the_1d_factors_is_the_oracle(p):
    orc = Oracle(p, 1, 1)
    e = dict(S=orc.shape_values(), D=orc.colloc_grad(), w=orc.qweights(), P1=orc.prolong_1d())
    M, K = ref.cell_matrices_1d(e)
    Mg, Kg = ref.assemble_1d(M, 2), ref.assemble_1d(K, 2)
    G, g = 2 * p + 1, orc.dof_grid(1)
    rng = np.random.default_rng(p)
    X = rng.standard_normal((G, G, G))
    free = np.zeros((G, G, G))
    free[1:-1, 1:-1, 1:-1] = 1
    h = orc.cell_size(1)   # merged coefficient of the Cartesian cube: h^3 / h^2
    Xf = free * X
    Y = h * (np.einsum("ai,bj,ck,abc->ijk", Mg, Mg, Kg, Xf) + np.einsum("ai,bj,ck,abc->ijk", Mg, Kg, Mg, Xf) +
             np.einsum("ai,bj,ck,abc->ijk", Kg, Mg, Mg, Xf))
    Y = free * Y + (1 - free) * X
    assert rel(orc.vmult(1, np.ascontiguousarray(X.ravel()[g])), Y.ravel()[g]) < 1e-12
    # embedding 1 -> 2^3 cells
    Pg = ref.embedding_1d(e["P1"], 1)
    xc = rng.standard_normal((p + 1,) * 3)
    fine = np.einsum("ai,bj,ck,ijk->abc", Pg, Pg, Pg, xc)
    g0 = orc.dof_grid(0)
    assert rel(orc.prolongate(1, np.ascontiguousarray(xc.ravel()[g0]), with_bc=False), fine.ravel()[g]) < 1e-13
    orc.close()


# ---------------------------------------------------------------------------------------------
# consistency of the reference
@pytest.fixture(scope="module")
def elements():
    out = {}
    for p in range(1, 5):
        sq = mg.Square(p, 1, 0)
        out[p] = ref.arrays_1d(sq)
        sq.close()
    return out


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_the_three_forms_agree_on_a_cartesian_box(elements, p):
    e = elements[p]
    cells, coef = (3, 2), np.array([1.3, 0.7, 0.0])
    w = e["w"]
    a = ref.Level(e, cells, coef)
    b = ref.Level(e, cells, coef, force_cellwise=True)
    cq = np.broadcast_to(coef[:, None, None] * np.outer(w, w)[None], (2, 3, 3, p + 1, p + 1)).copy()
    c = ref.Level(e, cells, coef_q=cq)
    x = np.random.default_rng(p).standard_normal(a.shape)
    assert rel(b.vmult(x), a.vmult(x)) < 1e-13 and rel(c.vmult(x), a.vmult(x)) < 1e-13
    assert rel(b.inv_diag(), a.inv_diag()) < 1e-13 and rel(c.inv_diag(), a.inv_diag()) < 1e-13
    assert rel(np.diag(a.dense()), 1 / a.inv_diag().ravel()) < 1e-13
    assert rel(a.dense() @ x.ravel(), a.vmult(x).ravel()) < 1e-13


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_sheared_operator_is_symmetric_and_restriction_is_the_transpose(elements, p):
    e = elements[p]
    prob = ref.Problem(e, A=[[1.0, 0.4], [0.2, 0.9]])
    assert prob.coef()[2] != 0
    A = ref.Level(e, (3, 2), prob.coef()).dense()
    assert np.abs(A - A.T).max() < 1e-13 * np.abs(A).max()
    assert np.linalg.eigvalsh(A).min() > 0
    c, f = ref.Level(e, (3, 2)), ref.Level(e, (6, 4))
    T = ref.Transfer(c, f)
    rng = np.random.default_rng(p)
    v, w = rng.standard_normal(c.shape), rng.standard_normal(f.shape)
    for bc in (False, True):
        lhs = np.vdot(T.prolongate(v, with_bc=bc), w)
        rhs = np.vdot(v, T.restrict_and_add(np.zeros(c.shape), w, with_bc=bc))
        assert lhs == pytest.approx(rhs, rel=1e-12)
    # a coarse polynomial is reproduced: the nodal values of a bilinear function
    xs, ys = np.linspace(0, 1, c.shape[1]), np.linspace(0, 1, c.shape[0])
    if p == 1:
        lin = 1 + 2 * xs[None, :] - 3 * ys[:, None]
        fx, fy = np.linspace(0, 1, f.shape[1]), np.linspace(0, 1, f.shape[0])
        assert rel(T.prolongate(lin), 1 + 2 * fx[None, :] - 3 * fy[:, None]) < 1e-14


# The dense solve written for the issue gave these L2 errors on [-0.9, 1]^2 with 8^2 and 16^2 cells.  They are the L2
# norm of the error itself; MultigridSolver::compute_l2_error, the provider and the reference's default divide by the
# square root of the volume, 1.9 here (the first run of this test showed exactly that factor at every degree).
DISCRETISATION = {1: (4.671e-1, 1.159e-1), 2: (5.653e-2, 8.598e-3), 3: (8.452e-3, 5.588e-4), 4: (8.497e-4, 2.878e-5)}


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_discretisation_error_of_the_dense_solve(elements, p):
    e = elements[p]
    prob = ref.Problem(e)
    err = []
    for n in (8, 16):
        L, h = ref.Level(e, (n, n)), 1.9 / n
        x = prob.dense_solution(L, h)
        err.append(prob.l2_error(L, h, x, normalised=False))
        assert err[-1] == pytest.approx(1.9 * prob.l2_error(L, h, x), rel=1e-12)
    print("p=%d  8^2: %.4e  16^2: %.4e  ratio %.3g" % (p, err[0], err[1], err[0] / err[1]))
    assert err[0] / err[1] > 0.8 * 2 ** (p + 1)
    np.testing.assert_allclose(err, DISCRETISATION[p], rtol=2e-3)   # three digits


def test_solver_reference_converges(elements):
    """the restated solver on levels 0..3 (8^2 cells): V-cycle PCG reaches the dense solution"""
    e = elements[2]
    s = ref.Solver(e, (1, 1), 4, 1.9)
    trace = s.solve()
    assert (trace[1:, 1] < 0.5 * trace[1:, 0]).all()   # one V-cycle per level at least halves the residual
    its, rate = s.solve_cg()
    assert 3 <= its <= 12 and len(s.cg_history) == its + 1
    exact = s.problem.dense_solution(s.level[-1], s.h[-1])
    assert rel(s.get_solution(), exact) < 1e-8
    fourth = ref.Solver(e, (1, 1), 4, 1.9, fourth_kind=True)
    assert fourth.solve_cg()[0] <= its + 2
