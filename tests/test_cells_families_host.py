"""CPU: the column families of the cell table do not disturb each other.  ``table_from_sums`` on the integers of
the restatements under tests/ for one small stack, with every family on at once, with every family alone and with every pair:
the columns are those of ``columns`` for the same switches, a family's columns hold the same values whichever other families
stand beside it, and a row that brings one value too few raises.  No device."""
import itertools

import numpy as np
import pytest

import cells_ref as ref
import drift_ref as dref
import flow_ref as fref
import gap_ref as gref
import hull_ref as href
import midline_ref as mref
import neighbors_ref as nref
import order_stats_ref as oref
import profile_ref as pref
import spots_ref as sref
from microbeseg_amd.inference import cells

T, H, W, TILE = 3, 16, 24, 8
CHANNELS = [0, 2]
PCT = (5, 50)
FAMILIES = ("shape", "channels", "links", "drift", "flow", "gap", "hull", "midline", "percentiles", "neighbors", "spots",
            "profile")
NEEDS = {"drift": ("links",), "flow": ("links", "drift"), "gap": ("links",)}       # what a family cannot stand without
TRACKS = ["track_id", "parent_track"]


def _stack():
    """3 frames of 16 x 24 with the cells 1, 2, 3 and 5 (id 4 is absent everywhere); all move by (1, 1) per frame, two of them
    touch, and cell 3 is missed in the middle frame: a gap to close"""
    lab = np.zeros((T, H, W), np.int64)
    boxes = {1: (1, 6, 1, 7), 2: (2, 7, 7, 13), 3: (8, 12, 2, 9), 5: (8, 13, 13, 20)}
    for t in range(T):
        for l, (r0, r1, c0, c1) in boxes.items():
            if (t, l) != (1, 3):
                lab[t, r0 + t:r1 + t, c0 + t:c1 + t] = l
    lab[:, 6, 6] = 0                                                # a notch: cell 1 is not convex
    rng = np.random.default_rng(5)
    img = rng.integers(0, 300, (T, 3, H, W)).astype(np.uint16)
    img[:, :, 3:5, 3:5] += 4000                                     # a focus on cell 1, in every channel
    img[:, 2, 10:12, 15:17] += 9000                                 # and one on cell 5 in channel 2
    return lab, img


@pytest.fixture(scope="module")
def integers():
    """every argument of ``table_from_sums`` for the stack with all families on, from the restatements; read only"""
    lab, img = _stack()
    off = ref.frame_tables(lab)
    assert int(off[-1]) == 15 and 4 not in lab and 3 not in lab[1]
    sel = np.ascontiguousarray(img[:, CHANNELS])
    raw = ref.measure(lab, off, sel)
    shift = dref.pick(dref.scores(lab, off, 2))
    assert shift[1:].tolist() == [[1, 1], [1, 1]]
    field = fref.pick(fref.scores(lab, off, shift, 1, TILE), shift)
    pred, ovl, gaps = gref.close_gaps(lab, off, *fref.links_field(lab, off, field, TILE), 1, 1, None, field, TILE)
    assert gaps.max() == 2                                          # cell 3 of frame 2 found cell 3 of frame 0
    area = raw["shape"][0].astype(np.int64)
    ranks = cells.percentile_ranks(area, PCT)[0]
    bg_ranks = cells.percentile_ranks(raw["bg_sums"][0, :, 0].astype(np.int64), PCT)[0]
    values, bg_values, status = oref.order_stats(lab, off, sel, raw["bbox"], ranks, bg_ranks)
    assert status == 0
    count, bg_count, recs = sref.reference(lab, off, img, CHANNELS, 500, 1)
    assert count.sum() >= 3
    given = {"links": dict(links=(pred, ovl)), "drift": dict(shift=shift), "flow": dict(field=field, tile=TILE),
             "gap": dict(gaps=gaps), "hull": dict(hull=href.hull(lab, off)), "midline": dict(midline=mref.midline(lab, off)[0]),
             "percentiles": dict(order_stats=(PCT, values, bg_values)), "neighbors": dict(neighbors=nref.neighbors(lab, off, 3)[0]),
             "spots": dict(spots=(1, count, bg_count, np.array(recs, cells.SPOT_RECORD))),
             "profile": dict(profile=pref.profile(lab, off, sel, raw["bbox"], cells._cell_directions(raw), 4))}
    return off, raw, ref.measure(lab, off), given


def _switches(on):
    return dict(channels=CHANNELS if _measured(on) else [], link="links" in on, drift="drift" in on, hull="hull" in on,
                midline="midline" in on, percentiles=PCT if "percentiles" in on else (), neighbors="neighbors" in on,
                spots="spots" in on, flow="flow" in on, gap="gap" in on, profile="profile" in on)


def _measured(on):
    return bool({"channels", "percentiles", "spots", "profile"} & set(on))


def _table(integers, on):
    """the table with the families ``on`` (and what they cannot stand without)"""
    off, raw, raw_plain, given = integers
    on = set(on) | {need for f in on for need in NEEDS.get(f, ())}
    args = {k: v for f in on for k, v in given.get(f, {}).items()}
    measured = _measured(on)
    return cells.table_from_sums(off, H, W, raw if measured else raw_plain, CHANNELS if measured else [], **args), on


def _own(family):
    """the columns of ``family``, from the constants of the module"""
    def per_channel(stencil):
        return [name.format(c=c) for c in CHANNELS for name in stencil]
    return {"shape": cells.SHAPE_COLUMNS, "channels": per_channel(cells.CHANNEL_COLUMNS), "links": cells.LINK_COLUMNS,
            "drift": cells.DRIFT_COLUMNS, "flow": cells.FLOW_COLUMNS, "gap": cells.GAP_COLUMNS, "hull": cells.HULL_COLUMNS,
            "midline": cells.MIDLINE_COLUMNS, "neighbors": cells.NEIGHBOR_COLUMNS, "spots": per_channel(cells.SPOT_COLUMNS),
            "percentiles": [name.format(p=p, c=c) for name in cells.PERCENTILE_COLUMNS for c in CHANNELS for p in PCT],
            "profile": ["axis_extent"] + per_channel(cells.PROFILE_COLUMNS)}[family]


def _same(family, big, big_on, small, small_on):
    """``family``'s columns hold the same in both tables.  track_id and parent_track are made of the links AND of pred_gap,
    where it is given: they are the links' between two tables that agree on ``gap``, and nobody's otherwise"""
    cols = [c for c in _own(family) if c not in TRACKS or ("gap" in big_on) == ("gap" in small_on)]
    assert cols and big[cols].equals(small[cols]), (family, sorted(big_on), sorted(small_on))


def test_all_families_at_once_have_the_columns_of_columns(integers):
    df, on = _table(integers, FAMILIES)
    assert list(df.columns) == cells.columns(**_switches(on)) and len(df) == 11
    assert len(set(df.columns)) == len(df.columns) == 13 + 6 * 2 + 4 + 4 + 2 + 1 + 10 + 10 + 2 * 2 * 2 + 10 + 4 * 2 + 1 + 3 * 2


@pytest.mark.parametrize("family", FAMILIES)
def test_a_family_alone_has_the_values_it_has_among_all(integers, family):
    everything, all_on = _table(integers, FAMILIES)
    alone, on = _table(integers, [family])
    assert list(alone.columns) == cells.columns(**_switches(on))
    _same(family, everything, all_on, alone, on)


@pytest.mark.parametrize("pair", list(itertools.combinations(FAMILIES, 2)), ids="-".join)
def test_every_pair_of_families(integers, pair):
    everything, all_on = _table(integers, FAMILIES)
    both, on = _table(integers, pair)
    assert list(both.columns) == cells.columns(**_switches(on))
    for family in pair:
        _same(family, everything, all_on, both, on)
        alone, alone_on = _table(integers, [family])
        _same(family, both, on, alone, alone_on)


def test_a_row_with_a_value_too_few_raises(integers, monkeypatch):
    outline = cells._outline
    monkeypatch.setattr(cells, "_outline", lambda area, h: outline(area, h)[:-1])
    with pytest.raises(RuntimeError, match="values for the"):
        _table(integers, ["hull", "midline"])
    _table(integers, ["midline"])                                   # the other families do not pass through it
