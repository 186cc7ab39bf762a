"""The square holds the 1D element data of FE_Q(p) by value, from the one make_basis the cube uses, and both providers
fill their seeded vectors with one function.  No GPU: the tables of both providers agree BITWISE at every degree, and the
seeded vectors are, bitwise, the splitmix64 rule restated in numpy on the provider's dof_grid."""
import numpy as np
import pytest

mg = pytest.importorskip("multigrid_amd")

MAX_DEGREE = 9  # MGX_MAX_DEGREE


@pytest.mark.parametrize("p", range(1, MAX_DEGREE + 1))
def test_square_and_cube_hold_the_same_element_data(p):
    sq, cube = mg.Square(p, 1, 0), mg.Cube(p, 1, 0)
    for name in ("shape_values", "colloc_grad", "qweights", "qpoints", "gll", "prolong_1d"):
        a, b = getattr(sq, name)(), getattr(cube, name)()
        assert a.shape == b.shape and a.dtype == b.dtype == np.float64, name
        assert a.tobytes() == b.tobytes(), name
    sq.close()
    cube.close()


def splitmix(seed, dof_grid):
    """entry i: splitmix64 of seed + golden * (grid id + 1), the upper 53 bits mapped to [-1, 1)"""
    u = np.uint64
    z = np.full(dof_grid.shape, seed, dtype=u) + u(0x9E3779B97F4A7C15) * (dof_grid.astype(u) + u(1))
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z ^= z >> u(31)
    return (z >> u(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


@pytest.mark.parametrize("seed", (42, 0xDEADBEEFCAFEF00D))
@pytest.mark.parametrize("make", (lambda: mg.Square(2, 1, 2), lambda: mg.Cube(2, 1, 1)), ids=("square", "cube"))
def test_seeded_vectors_are_the_splitmix_rule_on_the_dof_grid(make, seed):
    mesh = make()
    for l in range(mesh.n_levels):
        got, ref = mesh.seeded_vector(l, seed), splitmix(seed, mesh.dof_grid(l))
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), l
        assert (got >= -1).all() and (got < 1).all() and np.unique(got).size == got.size
    mesh.close()
