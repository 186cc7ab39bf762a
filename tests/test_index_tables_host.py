"""What the set-up code derives from a level's compressed index table (multigrid_amd/csrc/mgx_index_tables.hpp: first-owner
masks, greedy cell colours, multiplicity shifts of the children patches) without a device: tests/index_tables_check.cpp
builds small tables, prints them and what the three functions return -- built with AddressSanitizer and UBSan, no
library preloaded: the program has its own main --, and this test restates the three rules in numpy from the printed
tables and compares exactly.

Tables: structured boxes (2D 1x1, 3x2, 4x4; 3D 1x1x1, 3x2x1, 2x2x2) at degrees 1, 2, 3 in lexicographic and in Morton
cell order with one numbering -- at degree 1 the entries of the entities without DoFs hold garbage that looks like an
index --, one table per dimension with the boundary entities set to 0xFFFFFFFF; a fan of 32 and of 33 cells around one
vertex; one refinement of the 3x2 and 3x2x1 boxes (children in forest order and reversed); three quadrilaterals around
a vertex and three hexahedra around an edge with their children.

The same program runs the node rule and the row rule of that header and the tables that mgx_transfer_tables.hpp builds
with them, restated below in the same way, weights compared bit for bit: every node of p = 1..9 in 2D and 3D, every
layer and point of rows of 1 and 2 cells; the ordered assembly of the boxes above (with the constrained tables); the
patch table of one refinement of 3x2x1 and 2x2x2 at p = 1, 2, 3 (forest order and reversed, multiplicity and owner
weights with a foreign mask, one child tampered with: inconsistent) and the colouring by index mod 8 of 4x4x4 parents in
Morton (valid) and lexicographic order (not); block table, scratch CSR and brick cell lists of 8 bricks of 4x4x4 cells
at p = 2 and of 2x2x2 cells at p = 5, brick order identity and permuted; the interface rows of a 2x1x1 mesh refined once
at p = 1, 2, 3 (boundary free and constrained, nothing foreign and every other shared DoF) against kron(P1, P1, P1)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOXES = ["box2d-1x1", "box2d-3x2", "box2d-4x4", "box3d-1x1x1", "box3d-3x2x1", "box3d-2x2x2"]
BOX_TABLES = ["%s-p%d-%s" % (b, p, o) for b in BOXES for p in (1, 2, 3) for o in ("lex", "morton")]
CONSTRAINED = ["box2d-4x4-p2-constrained", "box3d-2x2x2-p2-constrained"]
REFINED = ["refined-box%dd%s-p%d" % (d, r, p) for d in (2, 3) for r in ("", "-reversed") for p in (1, 2, 3)]
THREE = ["three-around-2d", "three-around-3d"]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("index_tables") / "index_tables_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "index_tables_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, timeout=300).stdout.decode()
    vals = {}
    for line in out.splitlines():
        case, key, *v = line.split()
        vals.setdefault(case, {})[key] = np.array([int(a) for a in v], dtype=np.int64)
    assert vals["done"]["done"][0] == 1
    return vals


def entity_size(e, p):
    return ((p - 1) if e % 3 == 1 else 1) * ((p - 1) if e // 3 % 3 == 1 else 1) * ((p - 1) if e // 9 == 1 else 1)


def keys_of(c):
    """[n_cells][ne] first DoFs with -1 where the entity carries no DoF at this degree or its entry is no index"""
    dim, ne, n_cells, n_dofs, p = c["meta"][:5]
    idx = c["idx"].reshape(n_cells, ne).copy()
    has_dofs = np.array([entity_size(e, p) != 0 for e in range(ne)])
    idx[:, ~has_dofs] = -1
    idx[idx >= n_dofs] = -1
    return idx


def check_masks(c):
    """bit e of cell c iff c is the first cell that contains entity e; every entity has exactly one owner"""
    keys = keys_of(c)
    seen, want = set(), np.zeros(len(keys), dtype=np.int64)
    for cell, row in enumerate(keys):
        for e, k in enumerate(row):
            if k >= 0 and k not in seen:
                seen.add(k)
                want[cell] |= 1 << e
    assert np.array_equal(c["masks"], want)
    owners = {}
    for cell, row in enumerate(keys):
        for e, k in enumerate(row):
            if k >= 0 and c["masks"][cell] >> e & 1:
                owners[k] = owners.get(k, 0) + 1
    assert set(owners) == set(keys[keys >= 0]) and set(owners.values()) <= {1}


def check_colours(c):
    """the greedy rule restated; the classes share no key; order is a permutation sorted by colour, cells ascending"""
    keys = keys_of(c)
    more, n = c["colours"]
    used, colour = {}, []
    for row in keys:
        taken = set()
        for k in row[row >= 0]:
            taken |= used.get(k, set())
        col = next(k for k in range(33) if k not in taken)
        if col == 32:
            assert more == 1 and n == 0 and len(c["order"]) == 0 and not c["start"].any()
            return None
        colour.append(col)
        for k in row[row >= 0]:
            used.setdefault(k, set()).add(col)
    colour = np.array(colour)
    assert more == 0 and n == colour.max() + 1
    want_order = np.concatenate([np.flatnonzero(colour == k) for k in range(n)])
    assert np.array_equal(c["order"], want_order)
    assert np.array_equal(c["start"][:n + 1], np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=n))]))
    assert not c["start"][n + 1:].any()
    for k in range(n):
        in_class = keys[c["order"][c["start"][k]:c["start"][k + 1]]]
        in_class = in_class[in_class >= 0]
        assert len(np.unique(in_class)) == len(in_class)
    return n


@pytest.mark.parametrize("name", BOX_TABLES)
def test_structured_boxes(printed, name):
    c = printed[name]
    check_masks(c)
    assert c["out_of_range"][0] == 0
    cells = [int(a) for a in name.split("-")[1].split("x")]
    assert check_colours(c) == 2 ** sum(a >= 2 for a in cells)   # 4 in 2D, 8 in 3D where every direction has two cells
    if c["meta"][4] == 1:   # the garbage in the entries without DoFs looks like an index: skipped, not trusted
        idx = c["idx"].reshape(c["meta"][2], c["meta"][1])
        empty = [e for e in range(c["meta"][1]) if entity_size(e, 1) == 0]
        assert (idx[:, empty] < c["meta"][3]).all() and not (c["masks"][:, None] >> np.array(empty) & 1).any()


def test_both_cell_orders_number_the_same_entities(printed):
    for b in BOXES:
        for p in (1, 2, 3):
            lex, mor = keys_of(printed["%s-p%d-lex" % (b, p)]), keys_of(printed["%s-p%d-morton" % (b, p)])
            assert sorted(map(tuple, lex)) == sorted(map(tuple, mor))
    assert not np.array_equal(printed["box2d-4x4-p2-lex"]["idx"], printed["box2d-4x4-p2-morton"]["idx"])
    assert not np.array_equal(printed["box2d-4x4-p2-lex"]["order"], printed["box2d-4x4-p2-morton"]["order"])


@pytest.mark.parametrize("name", CONSTRAINED)
def test_constrained_entries_are_no_keys_and_are_reported(printed, name):
    c = printed[name]
    assert (c["idx"] == 0xFFFFFFFF).any() and c["out_of_range"][0] == 1
    check_masks(c)
    assert check_colours(c) == 2 ** c["meta"][0]


def test_fan_of_cells_around_one_vertex(printed):
    assert check_colours(printed["fan-32"]) == 32
    assert check_colours(printed["fan-33"]) is None
    assert list(printed["fan-33"]["colours"]) == [1, 0]
    check_masks(printed["fan-32"])
    check_masks(printed["fan-33"])


def patch_counts(c):
    """(shift wanted, irregular wanted): per parent and patch entity the number of parents whose children hold the
    entity's representative vertex -- low side: the low vertex of child 0, inside: its high vertex, high side: the high
    vertex of child 1"""
    dim, ne, n_fine, n_dofs, p, n_parents = c["meta"]
    idx, children = c["idx"].reshape(n_fine, ne), c["children"].reshape(n_parents, 2 ** dim)
    vertices = [e for e in range(ne) if all(e // 3 ** d % 3 != 1 for d in range(dim))]
    patch = [set(idx[children[pc]][:, vertices].ravel()) for pc in range(n_parents)]
    shift, irregular = np.zeros((n_parents, ne), dtype=np.int64), False
    for pc in range(n_parents):
        for e in range(ne):
            code = [e // 3 ** d % 3 for d in range(dim)]
            child = sum((code[d] == 2) << d for d in range(dim))
            vertex = sum((2 if code[d] else 0) * 3 ** d for d in range(dim))
            v = idx[children[pc, child], vertex]
            count = sum(v in s for s in patch)
            if count in (1, 2, 4, 8)[:dim + 1]:
                shift[pc, e] = int(np.log2(count))
            else:
                irregular = True
                shift[pc, e] = -1
    return shift, irregular


@pytest.mark.parametrize("name", REFINED)
def test_shifts_of_a_refined_box(printed, name):
    c = printed[name]
    want, irregular = patch_counts(c)
    assert not irregular and c["irregular"][0] == 0
    assert np.array_equal(c["shift"].reshape(want.shape), want)
    assert want.max() == 2   # four parents around an inner vertex of the 3x2 box, around an inner edge of the 3x2x1 box
    if "reversed" in name:
        assert not np.array_equal(c["children"], np.arange(len(c["children"])))


@pytest.mark.parametrize("name", THREE)
def test_three_cells_around_a_vertex_or_an_edge_are_irregular(printed, name):
    """the refusal in two dimensions, the owner-weights case in three; the regular entities still carry their shift"""
    c = printed[name]
    want, irregular = patch_counts(c)
    assert irregular and c["irregular"][0] == 1
    regular = want >= 0
    assert (~regular).any() and np.array_equal(c["shift"].reshape(want.shape)[regular], want[regular])


# ---- the node rule, the row rule and the tables built with them (mgx_transfer_tables.hpp) ----------------------------
INVALID = 0xFFFFFFFF


def node_entity(a, p):
    """(code, offset, run length) of node a of 0..p on a line"""
    return (0, 0, 1) if a == 0 else (2, 0, 1) if a == p else (1, a - 1, p - 1)


def cell_dofs(ix, dim, p):
    """DoFs of the (p + 1)^dim nodes of a cell in lexicographic order through its 3^dim entries, INVALID kept"""
    out = []
    for k in range(p + 1 if dim == 3 else 1):
        for j in range(p + 1):
            for i in range(p + 1):
                (cx, ox, lx), (cy, oy, ly), (cz, oz, _) = node_entity(i, p), node_entity(j, p), node_entity(k, p) if dim == 3 else (0, 0, 1)
                base = ix[(cz * 3 + cy) * 3 + cx]
                out.append(INVALID if base == INVALID else base + (oz * ly + oy) * lx + ox)
    return np.array(out, dtype=np.int64)


def layer_views(l, m):
    """the (cell, code) pairs of a row of m cells that are entity layer l: code k of cell c is layer 2 c + k"""
    return [(c, l - 2 * c) for c in range(m) if 0 <= l - 2 * c <= 2]


def block_views(e, m):
    """views of entity e of the (2 m + 1)^3 of a block of m^3 cells: (cell in the block, entity of that cell), z slowest"""
    L = 2 * m + 1
    return [((cz * m + cy) * m + cx, (kz * 3 + ky) * 3 + kx) for cz, kz in layer_views(e // (L * L), m)
            for cy, ky in layer_views(e // L % L, m) for cx, kx in layer_views(e % L, m)]


def point_layers(a, m, p):
    """what every cell of the row that holds point a says about it: (layer, offset, length); they agree"""
    said = {(2 * c + node_entity(a - c * p, p)[0],) + node_entity(a - c * p, p)[1:] for c in range(m) if 0 <= a - c * p <= p}
    assert len(said) == 1
    return said.pop()


@pytest.mark.parametrize("p", range(1, 10))
def test_node_rule_and_row_rule(printed, p):
    c = printed["rules-p%d" % p]
    assert np.array_equal(c["entity"].reshape(p + 1, 3), [node_entity(a, p) for a in range(p + 1)])
    for dim in (2, 3):
        ix = 1000 * np.arange(27, dtype=np.int64)
        ix[[5, 23]] = INVALID
        want = cell_dofs(ix, dim, p)
        assert np.array_equal(c["asked%d" % dim], want) and np.array_equal(c["walked%d" % dim], want)
        # every DoF of every entity exactly once
        valid = [e for e in range(3 ** dim) if ix[e] != INVALID]
        assert sorted(want[want != INVALID]) == sorted(1000 * e + t for e in valid for t in range(entity_size(e, p)))
        assert (want == INVALID).sum() == sum(entity_size(e, p) for e in (5, 23)[:dim - 1])
    for m in (1, 2):
        views = c["views%d" % m].reshape(2 * m + 1, 6)
        for l, (n, c0, k0, c1, k1, size) in enumerate(views):
            assert [(c0, k0), (c1, k1)][:n] == layer_views(l, m) and size == (p - 1 if l % 2 else 1)
        assert np.array_equal(c["points%d" % m].reshape(m * p + 1, 3), [point_layers(a, m, p) for a in range(m * p + 1)])


ASSEMBLED = ["%s-p%d-%s" % (b, p, o) for b in ("box2d-1x1", "box2d-3x2", "box3d-1x1x1", "box3d-3x2x1") for p in (1, 2, 3)
             for o in ("lex", "morton")] + CONSTRAINED


@pytest.mark.parametrize("name", ASSEMBLED)
def test_ordered_assembly(printed, name):
    c = printed[name]
    dim, ne, n_cells, n_dofs, p = c["meta"][:5]
    idx, nl = c["idx"].reshape(n_cells, ne), (p + 1) ** dim
    rows = [[] for _ in range(n_dofs)]
    for cell in range(n_cells):
        for l, d in enumerate(cell_dofs(idx[cell], dim, p)):
            if d != INVALID:
                rows[d].append(cell * nl + l)
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    assert np.array_equal(c["asm_start"], start)
    assert np.array_equal(c["asm_pos"], np.concatenate([np.array(r, dtype=np.int64) for r in rows] + [[0]]))  # (one of padding)
    pos = c["asm_pos"][:-1]
    # every local value of an entity that is not constrained exactly once; positions per DoF ascend
    valid = np.concatenate([cell * nl + np.flatnonzero(cell_dofs(idx[cell], dim, p) != INVALID) for cell in range(n_cells)])
    assert np.array_equal(np.sort(pos), valid)
    assert all((np.diff(pos[start[d]:start[d + 1]]) > 0).all() for d in range(n_dofs))
    if "constrained" in name:
        assert 0 < len(pos) < n_cells * nl and (np.diff(start) == 0).any()
    else:
        assert len(pos) == n_cells * nl and (np.diff(start) > 0).all()


PATCHES = ["patch-%s%s%s-p%d" % (b, r, o, p) for b in ("3x2x1", "2x2x2") for r in ("", "-reversed") for o in ("", "-owner")
           for p in (1, 2, 3)] + ["patch-2x2x2-tampered-p2"]


@pytest.mark.parametrize("name", PATCHES)
def test_patch_table(printed, name):
    c = printed[name]
    _, ne, n_fine, n_dofs, p, n_parents, owner_weights = c["meta"]
    idx, children = c["idx"].reshape(n_fine, 27), c["children"].reshape(n_parents, 8)
    shift, own, foreign = c["shift"].reshape(n_parents, 27), c["own"], c["foreign"]
    assert (len(foreign) == n_dofs and foreign.any()) if owner_weights else len(foreign) == 0
    want, consistent = np.zeros((n_parents, 125), dtype=np.int64), True
    for pc in range(n_parents):
        for e in range(125):
            el = (e % 5, e // 5 % 5, e // 25)
            views = [(children[pc, ch], ce) for ch, ce in block_views(e, 2)]
            bases = [idx[fc, ce] for fc, ce in views]
            consistent &= len(set(bases)) == 1
            owned = any(own[fc] >> ce & 1 for fc, ce in views)
            size = int(np.prod([p - 1 if l % 2 else 1 for l in el]))
            cls = sum((0 if l == 0 else 2 if l == 4 else 1) * 3 ** d for d, l in enumerate(el))
            sh = shift[pc, cls]
            if owner_weights:
                sh = 0 if owned and size and not foreign[bases[0]] else 1
            want[pc, e] = 0 if size == 0 else bases[0] | sh << 29 | int(owned) << 31
    assert c["consistent"][0] == consistent == ("tampered" not in name)
    assert np.array_equal(c["patch"].reshape(want.shape), want)
    if consistent and p > 1:
        # every fine DoF has exactly one owner bit over all patches
        owners = [w & 0x1FFFFFFF for w in want.ravel() if w >> 31]
        firsts = {idx[fc, e] for fc in range(n_fine) for e in range(27) if entity_size(e, p)}
        assert sorted(owners) == sorted(firsts)
        if owner_weights:  # exactly one parent restricts every entity that is not foreign
            restrict = [w & 0x1FFFFFFF for w in want.ravel() if w and not (w >> 29 & 3)]
            assert sorted(restrict) == sorted(b for b in firsts if not foreign[b])
    if "reversed" in name:
        assert not np.array_equal(c["children"], np.arange(8 * n_parents))


@pytest.mark.parametrize("p", (1, 2))
def test_parents_coloured_by_index_mod_8(printed, p):
    for order, want in (("morton", 1), ("lex", 0)):
        c = printed["mod8-%s-p%d" % (order, p)]
        keys = keys_of(c)
        keys[:, 13] = -1
        ok = True
        for colour in range(8):
            k = keys[colour::8]
            k = k[k >= 0]
            ok &= len(np.unique(k)) == len(k)
        assert c["coloured"][0] == ok == want


BRICKS = ["bricks-%s%s" % (b, o) for b in ("4x4x4-p2", "2x2x2-p5") for o in ("", "-permuted")]


@pytest.mark.parametrize("name", BRICKS)
def test_block_table_scratch_assembly_and_brick_cell_lists(printed, name):
    c = printed[name]
    _, ne, n_fine, n_dofs_fine, p, PB, nb, n_dofs, n_parents = c["meta"]
    idx, plain, order = c["idx_coarse"].reshape(n_parents, 27), c["idx_coarse_plain"].reshape(n_parents, 27), c["brick_order"]
    assert c["forest"][0] == 1 and (idx == INVALID).any() and ("permuted" in name) == (not np.array_equal(order, np.arange(nb)))
    CE1, ppb, CN = 2 * PB + 1, PB ** 3, PB * p + 1
    tab = np.zeros((nb, CE1 ** 3), dtype=np.int64)
    for sb in range(nb):
        for e in range(CE1 ** 3):
            views = [(ppb * order[sb] + q, ce) for q, ce in block_views(e, PB)]
            assert len({plain[pc, ce] for pc, ce in views}) == 1
            tab[sb, e] = idx[views[0]]
    assert np.array_equal(c["blocks"].reshape(tab.shape), tab)
    # the points of a block: DoF through the block table ...
    layers = [point_layers(a, PB, p) for a in range(CN)]
    dof = np.full((nb, CN, CN, CN), INVALID, dtype=np.int64)
    for sb in range(nb):
        for z, (ez, oz, _) in enumerate(layers):
            for y, (ey, oy, ly) in enumerate(layers):
                for x, (ex, ox, lx) in enumerate(layers):
                    w = tab[sb, (ez * CE1 + ey) * CE1 + ex]
                    if w != INVALID:
                        dof[sb, z, y, x] = w + (oz * ly + oy) * lx + ox
        # ... is the DoF of the parent's node there
        for q in range(ppb):
            qx, qy, qz = q % PB, q // PB % PB, q // (PB * PB)
            block = dof[sb, qz * p:qz * p + p + 1, qy * p:qy * p + p + 1, qx * p:qx * p + p + 1]
            assert np.array_equal(block.ravel(), cell_dofs(idx[ppb * order[sb] + q], 3, p))
    flat = dof.ravel()
    rows = [np.flatnonzero(flat == d) for d in range(n_dofs)]   # ascending position = ascending brick
    assert np.array_equal(c["cs_start"], np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    assert np.array_equal(c["cs_pos"], np.concatenate(rows))
    assert all((np.diff(r // CN ** 3) > 0).all() for r in rows) and max(len(r) for r in rows) == 8 and min(len(r) for r in rows) == 0
    # cell lists: brick colour by brick colour (one brick each), the cells m = q mod 8 of the brick
    cb = n_fine // nb
    want = [[order[g] * cb + m for m in range(q, cb, 8)] for g in range(8) for q in range(8)]
    assert np.array_equal(c["lists"], np.concatenate(want))
    assert np.array_equal(c["list_start"], np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert np.array_equal(np.sort(c["lists"]), np.arange(n_fine))
    keys = keys_of(c)
    for a, b in zip(c["list_start"][:-1], c["list_start"][1:]):
        in_list = keys[c["lists"][a:b]]
        in_list = in_list[in_list >= 0]
        assert len(np.unique(in_list)) == len(in_list)


INTERFACES = ["interface%s%s-p%d" % (b, h, p) for b in ("", "-constrained") for h in ("", "-half") for p in (1, 2, 3)]


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


@pytest.mark.parametrize("name", INTERFACES)
def test_interface_rows(printed, name):
    c = printed[name]
    _, ne, n_fine, n_dofs_fine, p, n_parents, n_dofs = c["meta"]
    n = p + 1
    idxf, idxc, children = c["idx"].reshape(n_fine, 27), c["idx_coarse"].reshape(n_parents, 27), c["children"].reshape(n_parents, 8)
    P1, shared, not_owned = bits(c["P1"]).reshape(2 * p + 1, n), c["shared"], c["not_owned"]
    assert (len(not_owned) == 0) == ("half" not in name) and len(shared) > 0 and c["verdict"][0] == 0
    # P = kron(P1, P1, P1) of every parent, weights multiplied x, y, z; dropped below 1e-14
    P, seen = {}, np.zeros((n_dofs_fine, n_dofs), dtype=bool)
    for pc in range(n_parents):
        coarse = cell_dofs(idxc[pc], 3, p).reshape(n, n, n)
        for ch in range(8):
            fine = cell_dofs(idxf[children[pc, ch]], 3, p).reshape(n, n, n)
            for iz, iy, ix in np.ndindex(n, n, n):
                d = fine[iz, iy, ix]
                F = ((ch & 1) * p + ix, (ch >> 1 & 1) * p + iy, (ch >> 2 & 1) * p + iz)
                for az, ay, ax in np.ndindex(n, n, n):
                    w = P1[F[0], ax] * P1[F[1], ay] * P1[F[2], az]
                    if d != INVALID and coarse[az, ay, ax] != INVALID and abs(w) >= 1e-14:
                        assert P.setdefault((d, coarse[az, ay, ax]), w) == w
    # the shared DoFs are those of the plane between the parents that are not constrained
    held = [set(cell_dofs(idxf[children[pc, ch]], 3, p)) for pc in range(2) for ch in range(8)]
    both = (set().union(*held[:8]) & set().union(*held[8:])) - {INVALID}
    assert sorted(both) == list(shared)
    ps, pc_, pw = c["p_start"], c["p_cdof"], bits(c["p_w"])
    assert len(ps) == len(shared) + 1 and ps[0] == 0 and ps[-1] == len(pc_) == c["verdict"][1]
    for i, d in enumerate(shared):
        row = {(d, cd): w for cd, w in zip(pc_[ps[i]:ps[i + 1]], pw[ps[i]:ps[i + 1]])}
        assert len(row) == ps[i + 1] - ps[i] and row == {k: w for k, w in P.items() if k[0] == d}
    owned = [d for d in shared if d not in set(not_owned)]
    rc, rs, rf, rw = c["r_cdof"], c["r_start"], c["r_fdof"], bits(c["r_w"])
    assert (np.diff(rc) > 0).all() and sorted(rc) == sorted({k[1] for k in P if k[0] in owned})
    assert len(rs) == len(rc) + 1 and rs[0] == 0 and rs[-1] == len(rf)
    for i, cd in enumerate(rc):
        row = {(fd, cd): w for fd, w in zip(rf[rs[i]:rs[i + 1]], rw[rs[i]:rs[i + 1]])}
        assert (np.diff(rf[rs[i]:rs[i + 1]]) > 0).all()   # in the order of the shared list, which ascends
        assert row == {k: w for k, w in P.items() if k[1] == cd and k[0] in owned}
    if "half" in name:
        # (degree 1 with the boundary constrained: one shared DoF, and every coarse DoF is constrained -- no entries)
        assert len(owned) == len(shared) // 2 and (len(rf) < len(pc_) or len(pc_) == 0)
    else:
        assert len(rf) == len(pc_)


def test_a_shared_dof_in_no_cell_is_reported(printed):
    c = printed["interface-lost-p2"]
    assert c["verdict"][0] == 1 and c["shared"][-1] == c["meta"][3] - 1 and len(c["p_start"]) == 0 and len(c["r_start"]) == 0
