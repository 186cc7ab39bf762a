"""What the set-up code derives from a level's compressed index table (multigrid_amd/csrc/mgx_index_tables.hpp: first-owner
masks, greedy cell colours, multiplicity shifts of the children patches) without a device: tests/index_tables_check.cpp
builds small tables, prints them and what the three functions return -- built with AddressSanitizer and UBSan, no
library preloaded: the program has its own main --, and this test restates the three rules in numpy from the printed
tables and compares exactly.

Tables: structured boxes (2D 1x1, 3x2, 4x4; 3D 1x1x1, 3x2x1, 2x2x2) at degrees 1, 2, 3 in lexicographic and in Morton
cell order with one numbering -- at degree 1 the entries of the entities without DoFs hold garbage that looks like an
index --, one table per dimension with the boundary entities set to 0xFFFFFFFF; a fan of 32 and of 33 cells around one
vertex; one refinement of the 3x2 and 3x2x1 boxes (children in forest order and reversed); three quadrilaterals around
a vertex and three hexahedra around an edge with their children."""
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
