"""The disc of the 2D provider (mgx_square_create_ball, Square(mapped="ball")) pinned on the CPU against the numpy
restatement of its mesh rule (tests/ball_reference_2d.py), the numpy laws of tests/nonlinear_reference_2d.py on it, and the
owner weights of the two-dimensional restriction on its level pair 1 -> 2 through a program of its own
(tests/ball_owner_weights_check.cpp, built with AddressSanitizer and UBSan).

NEWTON_CASES_BALL records, per case, the number of Newton steps to 1e-6 of the first residual norm with dense exact
solves (no step halved); test_gpu_ball_2d.py uses them as its yardstick."""
import os
import subprocess

import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")
import ball_reference_2d as br  # noqa: E402
import nonlinear_reference_2d as nr2  # noqa: E402
from test_nonlinear_reference_2d import boundary_state, reference, rel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (geometry, degree, n_refine, amplitude) -> N6
NEWTON_CASES_BALL = {("ball", 2, 1, 0.25): 3, ("ball", 2, 1, 1.0): 4, ("ball", 3, 2, 0.25): 4}


def make_ball(p, n_refine):
    return mg.Square(p, n_refine=n_refine, mapped="ball")


@pytest.mark.parametrize("p", [1, 2, 4])
def test_provider_tables(p):
    """cell nodes, counts, the constrained set, the index table, one coordinate per DoF, three cells around exactly four
    vertices of every level"""
    sq = make_ball(p, 2)
    n = p + 1
    for l in range(sq.n_levels):
        vertices, circle, cells = br.mesh(l)
        assert len(vertices) == br.count_vertices(l)
        nodes = sq.cell_nodes(l)
        assert np.abs(nodes - br.cell_nodes(vertices, circle, cells, sq.gll())).max() < 1e-14
        assert sq.n_cells(l) == 5 * 4 ** l and sq.n_dofs(l) == br.count_dofs(l, p)
        X = sq.dof_coordinates(l)
        at_radius_one = np.flatnonzero(np.abs(np.hypot(X[:, 0], X[:, 1]) - 1) < 1e-14)
        assert np.array_equal(np.sort(sq.constrained(l)), at_radius_one)
        assert sq.n_constrained(l) == at_radius_one.size
        plain = sq.idx9_plain(l).astype(np.int64)
        has_dofs = np.array([p > 1 or e in (0, 2, 6, 8) for e in range(9)])
        assert (plain[:, has_dofs] < sq.n_dofs(l)).all()
        dofs = nr2.cell_dofs(plain, p)
        assert np.array_equal(np.unique(dofs), np.arange(sq.n_dofs(l)))      # every DoF lies in a cell
        assert np.abs(X[dofs] - nodes).max() < 1e-14                         # shared DoFs have one coordinate
        con = sq.idx9(l).astype(np.int64)
        invalid = con == nr2.INVALID
        assert np.array_equal(con[~invalid], plain[~invalid])
        assert np.isin(plain[invalid & has_dofs[None, :]], sq.constrained(l)).all()
        corners = dofs.reshape(-1, n, n)[:, [0, 0, -1, -1], [0, -1, 0, -1]]
        count = np.bincount(corners.ravel(), minlength=sq.n_dofs(l))
        assert (count == 3).sum() == 4 and (count == 5).sum() == 0 and count.max() <= 4
        three = X[np.flatnonzero(count == 3)]
        assert np.abs(np.abs(three) - (1 - 1 / np.sqrt(2))).max() < 1e-15
        if l > 0:
            assert np.array_equal(sq.children(l), np.arange(sq.n_cells(l)).reshape(-1, 4))
    # no lattice, no grid, no Poisson problem
    for grid in (sq.cells_per_dim2, sq.cell_coords, sq.dof_grid, sq.weight_shift):
        with pytest.raises(mg._lib.MgxError) as e:
            grid(1)
        assert e.value.status == -4 and "disc" in str(e.value)
    lib = mg._lib.load()
    assert not lib.mgx_square_weight_shift(sq.h, 1) and not lib.mgx_square_cell_coords(sq.h, 1) and not lib.mgx_square_dof_grid(sq.h, 1)
    with pytest.raises(ValueError):
        sq.rhs(0)
    with pytest.raises(mg._lib.MgxError):
        sq.affine_metric(0)
    # the seeded vectors are keyed by the DoF index: the same generator on every level
    k = sq.n_dofs(1)
    assert np.array_equal(sq.seeded_vector(1, 5), sq.seeded_vector(2, 5)[:k]) and np.abs(sq.seeded_vector(1, 5)).max() <= 1
    assert not np.array_equal(sq.seeded_vector(1, 5), sq.seeded_vector(1, 6))
    sq.close()


@pytest.mark.parametrize("p", [2, 3, 4])
def test_area_converges_at_the_rate_of_the_degree(p):
    """sum of JxW_q against pi: per refinement the error of the isoparametric degree p falls by 2^(2p) (asserted: at
    least 0.8 of it between levels 1 and 2)"""
    sq = make_ball(p, 2)
    err = [abs(sq.jxw_q(l).sum() - np.pi) for l in (1, 2)]
    print("p=%d: area error %.3e (level 1), %.3e (level 2), ratio %.1f" % (p, err[0], err[1], err[0] / err[1]))
    assert err[0] / err[1] >= 0.8 * 2 ** (2 * p)
    sq.close()


@pytest.mark.parametrize("p", [1, 2, 4])
def test_geometry_and_unit_law(p):
    """unit_q and jxw_q are those the reference computes from the cell nodes; det J stays away from zero; the matrix of
    the unit law is symmetric and positive definite on the free DoFs"""
    sq = make_ball(p, 2)
    for l in range(sq.n_levels):
        ref = reference(sq, l, affine=False)
        assert rel(sq.unit_q(l), ref.U) < 1e-12
        assert rel(sq.jxw_q(l), ref.w) < 1e-12
        assert rel(sq.unit_law_coefficient(l), ref.U) < 1e-12
        assert 4 ** l * (ref.w / ref.wq[None, :]).min() >= 0.24
        d = sq.operator_desc(l)
        assert d.dim == 2 and bool(d.coef_q)
        A = ref.matrix(ref.coefficient(nr2.LAW_UNIT, None))[np.ix_(ref.free, ref.free)]
        assert np.abs(A - A.T).max() < 1e-13 * np.abs(A).max()
        assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0
    sq.close()


def test_tensor_is_the_derivative_of_the_residual():
    """[R(u - eps d) - R(u + eps d)] / (2 eps) = A(u) d: truncation eps^2 = 1e-10, rounding 1e-16 / eps = 1e-11"""
    sq = make_ball(2, 1)
    l = sq.max_level
    ref = reference(sq, l, affine=False)
    rng = np.random.default_rng(7)
    u = rng.uniform(-1, 1, sq.n_dofs(l))
    d = np.zeros(sq.n_dofs(l))
    d[ref.free] = rng.uniform(-1, 1, ref.free.size)
    eps = 1e-5
    fd = (ref.residual(nr2.LAW_MINIMAL_SURFACE, u - eps * d) - ref.residual(nr2.LAW_MINIMAL_SURFACE, u + eps * d)) / (2 * eps)
    ad = ref.apply(ref.coefficient(nr2.LAW_MINIMAL_SURFACE, u), d)
    ad[ref.constrained] = 0.0
    diff = np.abs(fd - ad).max() / np.abs(ad).max()
    print("ball p=2: central difference against A(u) d: %.3e" % diff)
    assert diff < 1e-6
    sq.close()


@pytest.mark.parametrize("p", [1, 2, 3])
def test_dense_embedding(p):
    """the mesh-agnostic P of ball_reference_2d: all parents of a fine DoF give the same row (asserted inside), rows sum
    to one (a constant is reproduced), and a coarse vertex value is carried to the fine vertex at the same place"""
    sq = make_ball(p, 2)
    for l in (1, 2):
        dc, df = nr2.cell_dofs(sq.idx9_plain(l - 1), p), nr2.cell_dofs(sq.idx9_plain(l), p)
        P = br.embedding(sq.prolong_1d(), sq.children(l), dc, df, sq.n_dofs(l - 1), sq.n_dofs(l))
        assert np.abs(P.sum(axis=1) - 1).max() < 1e-14
        # the coarse nodes are fine nodes: there the row is a unit vector, and the coordinates agree where the cells are
        # not curved differently on the two levels -- at the vertices
        n = p + 1
        vc = dc.reshape(-1, n, n)[:, [0, 0, -1, -1], [0, -1, 0, -1]].ravel()
        Xc, Xf = sq.dof_coordinates(l - 1), sq.dof_coordinates(l)
        for v in np.unique(vc):
            hit = np.flatnonzero(P[:, v] == 1.0)
            assert hit.size >= 1 and np.abs(Xf[hit] - Xc[v]).min() < 1e-15
    sq.close()


@pytest.mark.parametrize("p", [1, 2, 4])
def test_owner_weights_on_the_host(p, tmp_path):
    """level pair 1 -> 2 of the disc: the counts are irregular, the 9 bytes per parent are consistent, and, expanded to
    one weight per (parent, fine DoF), sum to exactly one over the parents of every fine DoF -- by the program's own
    expansion and by one in numpy from the printed bytes"""
    sq = make_ball(p, 2)
    exe, tables = str(tmp_path / "ball_owner_weights_check"), str(tmp_path / "tables.txt")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "ball_owner_weights_check.cpp")], check=True)
    children, idx = sq.children(2), sq.idx9_plain(2)
    with open(tables, "w") as f:
        f.write("%d %d %d %d\n" % (p, len(children), len(idx), sq.n_dofs(2)))
        f.write(" ".join(str(v) for v in children.ravel()) + "\n")
        f.write(" ".join(str(v) for v in idx.ravel()) + "\n")
    out = subprocess.run([exe, tables], check=True, capture_output=True, timeout=120).stdout.decode()
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.splitlines()}
    assert vals["done"] == ["1"] and vals["irregular"] == ["1"] and vals["consistent"] == ["1"]
    assert float(vals["sum_min"][0]) == 1.0 and float(vals["sum_max"][0]) == 1.0 and vals["parents_max"] == ["4"]
    weight = np.array([int(v) for v in vals["weight"]]).reshape(-1, 9)
    assert np.isin(weight, (0, 255)).all() and (weight[:, 4] == 0).all()
    # numpy: the byte of the parent entity a patch point lies in, summed per fine DoF
    n, m = p + 1, 2 * p + 1
    df = nr2.cell_dofs(idx, p)
    code = np.array([0 if a == 0 else (2 if a == 2 * p else 1) for a in range(m)])
    total, parents = np.zeros(sq.n_dofs(2)), np.zeros(sq.n_dofs(2), dtype=np.int64)
    for pc in range(len(children)):
        patch = np.empty((m, m), dtype=np.int64)
        for ch in range(4):
            ox, oy = (ch & 1) * p, (ch >> 1) * p
            patch[oy:oy + n, ox:ox + n] = df[children[pc, ch]].reshape(n, n)
        w = (weight[pc].reshape(3, 3)[code[:, None], code[None, :]] == 0).astype(np.float64)
        total[patch.ravel()] += w.ravel()
        parents[patch.ravel()] += 1
    assert np.array_equal(total, np.ones(sq.n_dofs(2)))
    assert (parents == 3).sum() == 4                      # the four fine vertices with three parents
    sq.close()


@pytest.mark.parametrize("case", sorted(NEWTON_CASES_BALL))
def test_newton_with_exact_linear_solves(case):
    _, p, n_refine, amplitude = case
    sq = make_ball(p, n_refine)
    l = sq.max_level
    ref = reference(sq, l, affine=False)
    _, norms, halvings = ref.newton(boundary_state(sq, l, amplitude), max_steps=12, tolerance=1e-13)
    print("ball p=%d, %d cells, A=%g: residual norms %s, halvings %s"
          % (p, sq.n_cells(l), amplitude, " -> ".join("%.2e" % r for r in norms), halvings))
    n6, n10 = nr2.steps_to(norms, 1e-6), nr2.steps_to(norms, 1e-10)
    assert n6 == NEWTON_CASES_BALL[case]
    assert n10 is not None and n10 <= n6 + 2
    assert not any(halvings)
    assert all(b < a for a, b in zip(norms, norms[1:]))
    sq.close()
