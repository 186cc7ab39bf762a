"""The standalone transfers (mgx_prolongate, mgx_restrict_and_add) on every route the dispatch can take, at every degree
p = 1..9, in fp64 and fp32, against the oracle and the lattice reference of tests/transfer_lattice.py.

Routes (mgx_transfer.hip launch_t; mgx_kernels.hip launch_prolongate / launch_restrict_add), each forced by its mesh,
thresholds and context options, and asserted from the trace lines of mgx_transfer_create:
  coloured  pipelined kernels, restriction in 8 colour launches (parent index mod 8): the 8 parents of ns = 1, level 1
  assembly  pipelined kernels, restriction in one launch through the ordered assembly of the coarse level (with
            constraints; atomic adds without): the 27 parents of ns = 3, level 0 -- not colourable by index mod 8 --
            on a coarse level without bricks (MGX_BRICK_MIN above every level)
  atomic    pipelined kernels, restriction in one launch with atomic adds (option restrict_atomic, a coarse level on
            bricks, which carries no assembly tables)
  v1        the first-version dense kernels (option transfer_v1), ns = 3
Each case runs prolongate (into a vector of NaN: a fine DoF never written fails), prolongate_and_add and
restrict_and_add (into non-zero data), with and without constraints.

Non-symmetric embeddings (p = 2..9): a Lagrange basis on the nodes (j/p)^1.3, passed through mg.Transfer on fresh
operators (mgx_transfer_create copies P1 into the basis blocks of both operators).  The pipelined kernels and the fused
forms read its even-odd form, which only a symmetric embedding has: such a transfer must run the first-version kernels
on every route, and the results must match the lattice reference built from the same P1.

Tolerances.  fp64: 1e-13 of the max-norm (as test_transfers).  fp32 (inputs rounded to fp32, compared with the fp64
reference): every output is a sum of products formed by three 1D sweeps; with unit round-off u = 2^-24 the classical
bound |fl(sum) - sum| <= gamma_k sum |terms|, gamma_k = k u / (1 - k u), holds for any summation order (atomics
included), so entry i is bounded by gamma_k (Q (x) Q (x) Q)|x| (+ |y| for the add forms), with Q the entrywise majorant
max(|P1[a,j]|, |P1[a,p-j]|, |P1[2p-a,j]|, |P1[2p-a,p-j]|) -- the even-odd form multiplies the halves (P1[a,j] +- P1[a,p-j])/2
with sums and differences of mirrored values, whose products are bounded by Q times those values.  Term count k:
three sweeps of at most 2p + 1 (restriction) or p + 1 (prolongation) products, plus two roundings per sweep in the
even-odd form (mirrored sums / differences in, halves combined out), three for P1 rounded to fp32 (one per factor), up
to 8 parent contributions and the old value for a restricted coarse DoF (9 additions), one addition for
prolongate_and_add, and the rounding of the stored result.  Weights 1/multiplicity are powers of two (exact)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("multigrid_amd")
from oracle_view import oracle_for  # noqa: E402
from transfer_lattice import LatticeTransfer, lagrange_embedding, skewed_nodes  # noqa: E402

U = 2.0 ** -24

ROUTES = {
    "coloured": dict(env={}, options={}),
    "assembly": dict(env={"MGX_BRICK_MIN": "4000000000"}, options={}),
    "atomic": dict(env={}, options={"restrict_atomic": 1}),
    "v1": dict(env={}, options={"transfer_v1": 1}),
}


def mesh_of(route, p):
    """(ns, nr): the transfer tested is the one onto the finest level nr"""
    if route in ("assembly", "v1"):
        return 3, 1
    if route == "atomic":  # a coarse level of at least one brick: 64 cells at p <= 4, 8 above
        return (1, 3) if p <= 4 else (1, 2)
    return 1, 2


def expected_lines(route, p, npar, symmetric):
    if route == "v1":
        return ["no patch table, first-version kernels (option transfer_v1)"]
    if not symmetric:
        return ["no patch table, first-version kernels (1D embedding not symmetric under reversal)",
                "fused residual + restriction no (1D embedding not symmetric under reversal)",
                "fused prolongation no"]
    out = ["patch table built, pipelined kernels"]
    if route == "coloured":
        out += ["coarse colouring yes", "restriction in 8 colour launches"]
    elif route == "assembly":
        out += ["coarse colouring no (%d parents, not a multiple of 8)" % npar,
                "restriction in one launch, ordered assembly with constraints, atomic adds without"]
    else:
        out += ["coarse colouring no (option restrict_atomic)", "restriction in one launch, atomic adds"]
    return out


_cubes, _oracles = {}, {}


def cube_of(p, ns, nr):
    if (p, ns, nr) not in _cubes:
        _cubes[(p, ns, nr)] = mg.Cube(p, ns, nr)
    return _cubes[(p, ns, nr)]


def oracle_of(p, ns, nr):
    if (p, ns, nr) not in _oracles:
        _oracles[(p, ns, nr)] = oracle_for(cube_of(p, ns, nr), p, ns, nr)
    return _oracles[(p, ns, nr)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for o in _oracles.values():
        o.close()
    for c in _cubes.values():
        c.close()
    _oracles.clear()
    _cubes.clear()


def majorant(P1):
    A = np.abs(P1)
    return np.maximum(np.maximum(A, A[:, ::-1]), np.maximum(A[::-1, :], A[::-1, ::-1]))


def run_case(monkeypatch, capfd, p, number, route, P1, symmetric):
    for k, v in ROUTES[route]["env"].items():
        monkeypatch.setenv(k, v)
    ns, nr = mesh_of(route, p)
    cube = cube_of(p, ns, nr)
    l = nr
    ctx = mg.Context(0, options=dict(ROUTES[route]["options"], trace=1))
    held = []  # device objects of this case, released in reverse order whatever happens
    try:
        vnum = mg.F32 if number == "f32" else mg.F64
        capfd.readouterr()
        ops = [mg.LaplaceOperator.from_cube(ctx, cube, k, number=vnum) for k in (l - 1, l)]
        held += ops
        tr = mg.Transfer(ops[0], ops[1], cube.children(l), P1)
        held.append(tr)
        trace = [s for s in capfd.readouterr().err.splitlines() if "transfer_create:" in s]

        cells = cube.cells_per_dim3(l - 1)[0]
        args = (cells, cube.dof_grid(l - 1), cube.dof_grid(l), cube.constrained(l - 1))
        lt, lq = LatticeTransfer(P1, *args), LatticeTransfer(majorant(P1), *args, majorant=True)
        orc = oracle_of(p, ns, nr) if symmetric else None
        xc, yc = cube.seeded_vector(l - 1, 11), cube.seeded_vector(l - 1, 13)
        xf = cube.seeded_vector(l, 12)
        if number == "f32":
            xc, yc, xf = (a.astype(np.float32).astype(np.float64) for a in (xc, yc, xf))
        nc, nf = xc.size, xf.size
        dc, df = ctx.vector(nc, vnum, xc), ctx.vector(nf, vnum, xf)
        held += [dc, df]
        k_p = 3 * (p + 1 + 2) + 3 + 1 + 1
        k_r = 3 * (2 * p + 1 + 2) + 3 + 9 + 1
        gamma = lambda k: k * U / (1 - k * U)  # noqa: E731

        def check(what, got, ref, mag, k, oref=None):
            got = got.astype(np.float64)
            assert np.isfinite(got).all(), "%s: entries never written" % what
            if number == "f64":
                assert rel(got, ref) < 1e-13, "%s: %g of the max-norm" % (what, rel(got, ref))
                if oref is not None:
                    assert rel(got, oref) < 1e-13, "%s: %g of the max-norm (oracle)" % (what, rel(got, oref))
            else:
                err = np.abs(got - ref) - gamma(k) * mag
                assert err.max() <= 1e-30, "%s: fp32 bound exceeded by %g at entry %d (%g of the max-norm)" % (
                    what, err.max(), int(err.argmax()), rel(got, ref))

        for wc in (False, True):
            out = ctx.vector(nf, vnum, np.full(nf, np.nan))
            held.append(out)
            tr.prolongate(out, dc, with_constraints=wc)
            check("prolongate(wc=%d)" % wc, out.download(), lt.prolongate(xc, with_constraints=wc),
                  lq.prolongate(np.abs(xc), with_constraints=wc), k_p,
                  orc.prolongate(l, xc, with_bc=wc) if orc else None)
            out.upload(xf)
            tr.prolongate_and_add(out, dc, with_constraints=wc)
            check("prolongate_and_add(wc=%d)" % wc, out.download(), lt.prolongate(xc, xf, with_constraints=wc),
                  lq.prolongate(np.abs(xc), np.abs(xf), with_constraints=wc), k_p,
                  orc.prolongate(l, xc, fine=xf, with_bc=wc) if orc else None)
            outc = ctx.vector(nc, vnum, yc)
            held.append(outc)
            tr.restrict_and_add(outc, df, with_constraints=wc)
            check("restrict_and_add(wc=%d)" % wc, outc.download(), lt.restrict_and_add(yc, xf, with_constraints=wc),
                  lq.restrict_and_add(np.abs(yc), np.abs(xf), with_constraints=wc), k_r,
                  orc.restrict_and_add(l, yc, xf, with_bc=wc) if orc else None)
    finally:
        for obj in reversed(held):
            if isinstance(obj, mg.DeviceVector):
                obj.free()
            else:
                obj.clear()
        ctx.close()

    # the route this case claims is the one that ran (checked after the results, which are the point)
    for e in expected_lines(route, p, cube.n_cells(l - 1), symmetric):
        assert any(e in s for s in trace), "route %s: no trace line %r in %s" % (route, e, trace)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", range(1, 10))
def test_transfer_route(monkeypatch, capfd, p, number, route):
    """Gauss-Lobatto embedding (the cube's prolong_1d) on each route"""
    run_case(monkeypatch, capfd, p, number, route, cube_of(p, *mesh_of(route, p)).prolong_1d(), True)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("number", ["f64", "f32"])
@pytest.mark.parametrize("p", range(2, 10))
def test_transfer_route_non_symmetric_embedding(monkeypatch, capfd, p, number, route):
    """A Lagrange embedding on nodes that are not mirror-symmetric: the first-version kernels on every route"""
    run_case(monkeypatch, capfd, p, number, route, lagrange_embedding(skewed_nodes(p)), False)
