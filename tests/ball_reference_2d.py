"""numpy restatement of the disc mesh of include/mgx_square.h (mgx_square_create_ball: GridGenerator::hyper_ball in two
dimensions with a SphericalManifold on the boundary and MappingQGeneric(p), minimal_surface/program.cc:630-634, :226) and
of the level transfer of a mesh whose parents are glued in any way: the vertices by recursion, the cell nodes by the edge
rule and transfinite interpolation, the embedding P as a dense matrix assembled parent by parent from the children
table, the DoFs of the cells of both levels and kron(P1, P1).  Nothing here is taken from the provider but the tables a
test hands in.  test_ball_reference_2d.py pins it, test_gpu_ball_2d.py compares the device against it.

TEST INFRASTRUCTURE ONLY.

The mesh.  Eight vertices: C(s, t) = (s i, t i) and O(s, t) = (s o, t o) with o = 1 / sqrt 2, i = 1 - o, numbered
C(-1,-1), C(1,-1), C(-1,1), C(1,1), O likewise.  Five cells with the vertices v00, v10, v01, v11 (local x fastest):
centre, right, top, left, bottom -- right-handed, every shared edge running the same way in both of its cells.
Refinement: the children of cell c are 4c .. 4c+3 with child = x + 2y; a new vertex on an edge is the straight midpoint,
projected to the circle if both ends lie on it; the new vertex of a cell is 1/2 (sum of the four edge midpoints) - 1/4
(sum of the four vertices)."""
import numpy as np

BLOCKS = np.array([[0, 1, 2, 3], [1, 5, 3, 7], [2, 3, 6, 7], [0, 2, 4, 6], [0, 4, 1, 5]])


def coarse_mesh():
    """(vertices [8, 2], on_circle [8], cells [5, 4])"""
    o = 1 / np.sqrt(2.0)
    i = 1 - o
    sign = np.array([[-1, -1], [1, -1], [-1, 1], [1, 1]], dtype=np.float64)
    return np.concatenate([i * sign, o * sign]), np.arange(8) >= 4, BLOCKS.copy()


def refine(vertices, on_circle, cells):
    vertices, on_circle = [tuple(v) for v in vertices], list(on_circle)
    mid = {}

    def midpoint(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            m = 0.5 * (np.array(vertices[a]) + np.array(vertices[b]))
            circle = on_circle[a] and on_circle[b]
            if circle:
                m = m / np.hypot(m[0], m[1])
            vertices.append(tuple(m))
            on_circle.append(circle)
            mid[key] = len(vertices) - 1
        return mid[key]

    fine = []
    for v in cells:
        mb, mt, ml, mr = midpoint(v[0], v[1]), midpoint(v[2], v[3]), midpoint(v[0], v[2]), midpoint(v[1], v[3])
        centre = 0.5 * sum(np.array(vertices[k]) for k in (mb, mt, ml, mr)) - 0.25 * sum(np.array(vertices[k]) for k in v)
        vertices.append(tuple(centre))
        on_circle.append(False)
        c = len(vertices) - 1
        fine += [[v[0], mb, ml, c], [mb, v[1], c, mr], [ml, c, v[2], mt], [c, mr, mt, v[3]]]
    return np.array(vertices), np.array(on_circle), np.array(fine)


def mesh(level):
    m = coarse_mesh()
    for _ in range(level):
        m = refine(*m)
    return m


def cell_nodes(vertices, on_circle, cells, gll):
    """[n_cells, (p+1)^2, 2], x fastest: linear on a straight edge, at angles linear in the node parameter on an edge of the
    boundary, X(s, u) = (1-u) B(s) + u T(s) + (1-s) L(u) + s R(u) - bilinear(corners) inside"""
    g = np.asarray(gll, dtype=np.float64)
    n = g.size

    def edge(a, b):
        xa, xb = vertices[a], vertices[b]
        if on_circle[a] and on_circle[b]:
            ta = np.arctan2(xa[1], xa[0])
            dt = np.arctan2(xb[1], xb[0]) - ta
            dt -= 2 * np.pi * np.round(dt / (2 * np.pi))
            out = np.stack([np.cos(ta + g * dt), np.sin(ta + g * dt)], axis=1)
        else:
            out = xa[None, :] + g[:, None] * (xb - xa)[None, :]
        out[0], out[-1] = xa, xb
        return out

    s, u = g[None, :, None], g[:, None, None]
    out = np.empty((len(cells), n, n, 2))
    for c, v in enumerate(cells):
        B, T, L, R = edge(v[0], v[1]), edge(v[2], v[3]), edge(v[0], v[2]), edge(v[1], v[3])
        x0, x1, x2, x3 = (vertices[k] for k in v)
        X = (1 - u) * B[None] + u * T[None] + (1 - s) * L[:, None] + s * R[:, None] \
            - ((1 - s) * (1 - u) * x0 + s * (1 - u) * x1 + (1 - s) * u * x2 + s * u * x3)
        X[0], X[-1], X[:, 0], X[:, -1] = B, T, L, R
        out[c] = X
    return out.reshape(len(cells), n * n, 2)


def count_vertices(level):
    """distinct vertices of level l: 5 4^l + 2^(l+1) + 1"""
    return 5 * 4 ** level + 2 ** (level + 1) + 1


def count_dofs(level, p):
    """V + (p - 1) E + (p - 1)^2 C with E = 2 C + 2^(l+1) (Euler: V - E + C = 1)"""
    C = 5 * 4 ** level
    return count_vertices(level) + (p - 1) * (2 * C + 2 ** (level + 1)) + (p - 1) ** 2 * C


def embedding(P1, children, dofs_coarse, dofs_fine, n_coarse, n_fine):
    """dense P [n_fine, n_coarse] of a level pair: per parent the (2p+1)^2 points of its children patch get the rows of
    kron(P1, P1) in the parent's DoFs (dofs_*: [n_cells, (p+1)^2] without constrained entries, x fastest).  All parents
    of a fine DoF must give the same row (the embedding is interpolatory: a fine DoF on a shared entity couples to the
    coarse DoFs of that entity alone)."""
    P1 = np.asarray(P1, dtype=np.float64)
    m, n = P1.shape
    p = n - 1
    K = np.kron(P1, P1)  # [b m + a, j n + i]
    children = np.asarray(children).reshape(-1, 4)
    P = np.zeros((n_fine, n_coarse))
    seen = np.zeros(n_fine, dtype=bool)
    for pc in range(children.shape[0]):
        patch = np.full((m, m), -1, dtype=np.int64)
        for ch in range(4):
            ox, oy = (ch & 1) * p, (ch >> 1) * p
            d = dofs_fine[children[pc, ch]].reshape(n, n)
            old = patch[oy:oy + n, ox:ox + n]
            assert ((old < 0) | (old == d)).all()   # the children agree on what they share
            patch[oy:oy + n, ox:ox + n] = d
        rows = np.zeros((m * m, n_coarse))
        rows[:, dofs_coarse[pc]] = K
        fd = patch.ravel()
        again = seen[fd]
        assert np.abs(P[fd[again]] - rows[again]).max(initial=0.0) < 1e-15
        P[fd[~again]] = rows[~again]
        seen[fd] = True
    assert seen.all()
    return P


def prolongate(P, coarse, constrained_coarse=None, fine=None):
    """fine (None: zero) + P coarse; constrained_coarse: those entries of coarse are read as zero"""
    x = np.array(coarse, dtype=np.float64)
    if constrained_coarse is not None:
        x[constrained_coarse] = 0.0
    out = P @ x
    return out if fine is None else np.asarray(fine, dtype=np.float64) + out


def restrict_and_add(P, coarse, fine, constrained_coarse=None):
    """coarse + P^T fine; constrained_coarse: those rows are skipped"""
    out = np.asarray(coarse, dtype=np.float64) + P.T @ np.asarray(fine, dtype=np.float64)
    if constrained_coarse is not None:
        out[constrained_coarse] = np.asarray(coarse, dtype=np.float64)[constrained_coarse]
    return out
