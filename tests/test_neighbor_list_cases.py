"""The neighbour-list cases of ``tests/neighbor_list_cases.py`` on the CPU: every case has the property it was built for, keeps
its distance from the cutoffs, and the float64 enumeration they are compared with is checked against an independent search (the
scipy KD-tree stand-in of ``nequip_amd.utils.synthetic``) and shown to tell a float32 evaluation apart."""
import numpy as np
import pytest

import neighbor_list_cases as nc


@pytest.mark.parametrize("name", nc.NAMES)
def test_case_has_its_property_and_margin(name):
    """``make_case`` asserts the property of the case (see the builder); the margin bar holds for every case but ``exact_grid``,
    whose boundary pairs are deliberate and whose values are exact."""
    case = nc.make_case(name)
    row = nc.table_row(case)
    print("\n" + row)
    assert row in nc.__doc__, "the table in the docstring of neighbor_list_cases.py is out of date"
    e = nc.enumerate_edges(case)
    assert e.dtype == np.int64 and e.shape[1] == 5 and len(np.unique(e, axis=0)) == len(e)
    assert np.array_equal(e, nc.sort_rows(e)) and not e.flags.writeable
    rev = nc.sort_rows(np.concatenate([e[:, [1, 0]], -e[:, 2:]], 1))
    assert np.array_equal(rev, e), "the list of a frame is symmetric under (i, j, S) -> (j, i, -S)"
    m = nc.margin(case)
    if name == "exact_grid":
        assert m == 0.0
    else:
        assert m >= nc.MARGIN_MIN


def test_cases_reach_the_loops_they_are_for():
    g = {n: nc.expected_grid(nc.make_case(n), nc.make_case(n).num_atoms + 8) for n in nc.NAMES}
    assert sum(v.max_run > 128 for v in g.values()) >= 2 and sum(64 < v.max_run <= 128 for v in g.values()) >= 1  # walk: 2nd, 3rd trip
    assert sum(v.max_bin > 128 for v in g.values()) >= 2  # rank sort of a bin: third trip
    assert any(v.capped for v in g.values()) and max(v.halvings for v in g.values()) >= 20
    assert any(max(v.reach) >= 3 for v in g.values()) and any(v.reach == (2, 2, 2) for v in g.values())
    deg = {n: np.bincount(nc.enumerate_edges(nc.make_case(n))[:, 0], minlength=nc.make_case(n).num_atoms) for n in nc.NAMES}
    assert sum(d.max() > 128 for d in deg.values()) >= 3  # CSR rows for the third trip of the partner scan / owner ballots
    assert any(d.min() == 0 for d in deg.values())


@pytest.mark.parametrize("name", nc.TYPED_NAMES)
def test_typed_cases(name):
    case = nc.typed_case(name)
    m = nc.margin(case)
    print(f"\n{case.name:<28} margin {m:7.1e}  kept {len(nc.typed_edges(case))} of {len(nc.enumerate_edges(case))}")
    assert m >= nc.MARGIN_MIN
    assert {case.r_max, 0.6 * case.r_max, 0.0} == set(case.table.reshape(-1).tolist())
    e = nc.enumerate_edges(case)
    keep = nc.typed_keep(case, e)
    pair = case.types[e[:, 0]] * nc.NUM_TYPES + case.types[e[:, 1]]
    assert keep[pair == 0].all() and keep[pair == 8].all()  # same type: r_max
    assert 0 < keep[pair == 2].sum() < (pair == 2).sum()  # 0 <- 2: 0.6 r_max cuts the row
    assert (pair == 6).any() and not keep[pair == 6].any()  # 2 <- 0: cutoff 0 keeps nothing that has a length


@pytest.mark.parametrize("name", nc.NAMES)
def test_enumeration_against_the_kdtree_search(name):
    """The enumerator is not self-certifying: where the KD-tree stand-in can represent the case (``kdtree_supported``: no cell,
    or fully periodic with the atoms spread over less than one cell and no pair at exactly r_max) it gives the same array.
    Supported: crowded_single_bin, dense_640, blob_no_cell, cluster_on_corner, clipped_1024, skewed, one_atom_images,
    minus_epsilon; the others have mixed periodicity (slab_crowded), atoms spread over more than one cell (thin_x, left_handed,
    coincident, exact_grid) or boundary pairs (exact_grid)."""
    from nequip_amd.utils import synthetic as syn

    case = nc.make_case(name)
    supported = ("crowded_single_bin", "dense_640", "blob_no_cell", "cluster_on_corner", "clipped_1024", "skewed", "one_atom_images",
                 "minus_epsilon")
    assert nc.kdtree_supported(case) == (name in supported)
    if name not in supported:
        return
    ei, sh = syn.neighbor_list(case.pos, case.r_max, case.cell, pbc=case.cell is not None)
    assert np.array_equal(sh, np.round(sh))
    got = nc.sort_rows(np.concatenate([ei.T, sh.astype(np.int64)], 1))
    assert np.array_equal(got, nc.enumerate_edges(case))


def test_a_float32_evaluation_is_told_apart():
    """The comparison can discriminate: the same enumeration in float32 gives another set on ``dense_640``, or the margin rule
    rejects the case for float32.  The rule, as for float64: an error of about 10 ulp of the largest coordinate, relative to r_max,
    and two orders of room: 100 * 10 * 2^-24 * 18 A / 5 A = 2.1e-4."""
    case = nc.make_case("dense_640")
    e32, e64 = nc.enumerate_edges_float32(case), nc.enumerate_edges(case)
    differs = e32.shape != e64.shape or not np.array_equal(e32, e64)
    bar32 = 100.0 * 10.0 * 2.0 ** -24 * float(np.abs(case.pos).max()) / case.r_max
    print(f"\nfloat32 set differs: {differs}; margin {nc.margin(case):.1e} against a float32 bar of {bar32:.1e}")
    assert differs or nc.margin(case) < bar32
