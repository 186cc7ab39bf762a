"""The numpy restatement of the solution-dependent coefficient on curved cells (tests/nonlinear_reference_mapped.py)
pinned on the CPU: its geometry, computed from the cell nodes, is the provider's; on the sheared box it agrees with the
affine restatement (two routes to one answer); the minimal-surface tensor is the derivative of the minimal-surface
residual on curved cells; Newton's method with exact linear solves converges.

NEWTON_CASES_MAPPED records, per case, the number of Newton steps to 1e-6 of the first residual norm as measured with the
project's own tables (dense exact solves, no halved step in any of them); test_gpu_nonlinear_mapped.py uses them as its
yardstick.  The whole shell at p = 2, one refinement: amplitude 1 takes a halved step in the second Newton step,
0.5 and 0.25 take none -- 0.5 is the case."""
import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")
import nonlinear_reference as nr  # noqa: E402
import nonlinear_reference_mapped as nm  # noqa: E402

# (geometry, degree, n_refine, amplitude) -> N6: steps until the residual norm is below 1e-6 of the first one
NEWTON_CASES_MAPPED = {
    ("shell_sector", 2, 2, 0.25): 4,
    ("shell_sector", 3, 1, 0.25): 4,
    ("shell_sector", 3, 2, 0.25): 4,
    ("shell_sector", 4, 1, 0.25): 4,
    ("sheared", 2, 2, 1.0): 4,
    ("shell6", 2, 1, 0.5): 5,
}


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("geometry", sorted(nm.GEOMETRIES))
@pytest.mark.parametrize("p", [2, 3])
def test_geometry_is_the_providers(geometry, p):
    cube = nm.make_cube(mg, geometry, p, 1)
    for l in range(cube.n_levels):
        ref = nm.mapped_reference(cube, l)
        du, dw = rel(ref.unit_tensor(), cube.coef_q(l)), rel(ref.jxwq, cube.jxw_q(l))
        print("%s p=%d level %d: unit tensor %.2e, JxW %.2e" % (geometry, p, l, du, dw))
        assert du < 1e-12 and dw < 1e-12
    cube.close()


def test_cartesian_cube_has_no_per_point_geometry():
    cube = mg.Cube(2, 1, 1)
    assert cube.jxw_q(0) is None and cube.coef_q(0) is None
    cube.close()


@pytest.mark.parametrize("p,n_refine", [(2, 2), (3, 1)])
def test_sheared_box_agrees_with_the_affine_reference(p, n_refine):
    sheared = nm.make_cube(mg, "sheared", p, n_refine)
    box = mg.Cube(p, n_refine=n_refine, box=(1, 1, 1), origin=-0.9, h0=1.9)
    l = sheared.max_level
    assert np.array_equal(sheared.idx27(l), box.idx27(l)) and np.array_equal(sheared.idx27_plain(l), box.idx27_plain(l))
    ref = nm.mapped_reference(sheared, l)
    metric, det = box.affine_metric(l, nm.SHEAR)
    aff = nr.NonlinearReference(p, box.shape_values(), box.colloc_grad(), box.qweights(), box.idx27(l), box.idx27_plain(l),
                                box.n_dofs(l), metric, det)
    u = np.random.default_rng(11).uniform(-1, 1, box.n_dofs(l))
    for law in (nr.LAW_UNIT, nr.LAW_MINIMAL_SURFACE):
        dc, dr = rel(ref.coefficient(law, u), aff.coefficient(law, u)), rel(ref.residual(law, u), aff.residual(law, u))
        print("p=%d law %d: tensor %.2e, residual %.2e" % (p, law, dc, dr))
        assert dc < 1e-12 and dr < 1e-12
    # the node coordinates are those of the affine map of the box (about the origin of the reference box)
    x = sheared.dof_coordinates(l)
    assert np.abs(x - box.dof_coordinates(l) @ nm.SHEAR.T).max() < 1e-14
    sheared.close()
    box.close()


@pytest.mark.parametrize("p,n_refine", [(2, 2), (3, 1)])
def test_tensor_is_the_derivative_of_the_residual_on_curved_cells(p, n_refine):
    cube = nm.make_cube(mg, "shell_sector", p, n_refine)
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    rng = np.random.default_rng(7)
    # |grad u| of order one on cells of size 1/4 .. 1/2
    u = 0.2 * rng.uniform(-1, 1, cube.n_dofs(l))
    v = np.zeros(cube.n_dofs(l))
    v[ref.free] = rng.uniform(-1, 1, ref.free.size)
    eps = 1e-6
    fd = (ref.residual(nr.LAW_MINIMAL_SURFACE, u + eps * v) - ref.residual(nr.LAW_MINIMAL_SURFACE, u - eps * v)) / (2 * eps)
    av = ref.apply(ref.coefficient(nr.LAW_MINIMAL_SURFACE, u), v)
    av[ref.constrained] = 0.0
    diff = np.abs(fd + av).max() / np.abs(av).max()
    print("p=%d: relative difference of the central difference and -A(u) v: %.3e" % (p, diff))
    assert diff < 1e-8
    cube.close()


def test_unit_law_residual_is_minus_the_operator():
    """- A_unit u with the boundary values read: what compute_residual of the linear operator gives without a source"""
    cube = nm.make_cube(mg, "shell6", 2, 1)
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    u = nm.smooth_state(cube, l)
    plain = nm.MappedNonlinearReference(2, cube.shape_values(), cube.colloc_grad(), cube.qweights(), cube.idx27_plain(l),
                                        cube.idx27_plain(l), cube.n_dofs(l), cube.cell_nodes(l))
    want = -plain.apply(plain.unit_tensor(), u)
    want[ref.constrained] = 0.0
    assert rel(ref.residual(nr.LAW_UNIT, u), want) < 1e-12
    cube.close()


@pytest.mark.parametrize("case", sorted(NEWTON_CASES_MAPPED))
def test_newton_with_exact_linear_solves(case):
    geometry, p, n_refine, amplitude = case
    cube = nm.make_cube(mg, geometry, p, n_refine)
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    _, norms, halvings = ref.newton(nm.boundary_state(cube, l, amplitude), max_steps=12, tolerance=1e-13)
    print("%s p=%d, %d cells, A=%g: residual norms %s, halvings %s"
          % (geometry, p, cube.n_cells(l), amplitude, " -> ".join("%.2e" % r for r in norms), halvings))
    n6, n10 = nr.steps_to(norms, 1e-6), nr.steps_to(norms, 1e-10)
    assert n6 == NEWTON_CASES_MAPPED[case]
    assert n10 is not None and n10 <= n6 + 2
    assert all(b < a for a, b in zip(norms, norms[1:]))
    assert not any(halvings)
    cube.close()


def test_the_whole_shell_takes_a_halved_step_at_amplitude_one():
    """why NEWTON_CASES_MAPPED has the shell at amplitude 0.5: the largest of 1, 0.5, 0.25 without a halved step"""
    cube = nm.make_cube(mg, "shell6", 2, 1)
    l = cube.max_level
    ref = nm.mapped_reference(cube, l)
    _, _, halvings = ref.newton(nm.boundary_state(cube, l, 1.0), max_steps=12, tolerance=1e-13)
    assert any(halvings)
    cube.close()
