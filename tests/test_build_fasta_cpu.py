"""skm_build_add_fasta on the CPU: the entry points exist with their argument counts, the selected
layout the GPU tests expect is right by hand-written expectations, and every planted tile-edge
input holds the edge it is named for (proven from its bytes)."""
import os
import re

import numpy as np
import pytest

import build_fasta_util as bu
import fasta_device_util as fu
from conftest import ROOT

UNDEF = bu.UNDEF


def _header_args(name):
    """the argument count of `name`'s declaration in include/skm.h"""
    header = open(os.path.join(ROOT, "include", "skm.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,nargs", [("skm_build_add_fasta", 8), ("skm_build_debug_input", 7)])
def test_new_symbols_and_argument_counts(skm, name, nargs):
    assert hasattr(skm.lib(), name), name
    assert name in skm._SIGS and len(skm._SIGS[name][1]) == nargs
    assert _header_args(name) == nargs
    assert callable(getattr(skm.SignatureBuilder, {"skm_build_add_fasta": "add_fasta",
                                                   "skm_build_debug_input": "debug_input"}[name]))


def test_counter_list_gains_add_fasta_us_at_its_end(skm):
    import inspect
    src = inspect.getsource(skm.SignatureBuilder.counters)
    names = re.findall(r'"([a-z0-9_]+)"', src)
    assert names[-1] == "add_fasta_us" and names[-2] == "groupby_batches" and len(names) == 51
    assert names[26] == "add_batch_us" and names[31] == "add_pack_us" and names[32] == "add_dma_wait_us"
    assert np.dtype(skm.SEQ_META_DTYPE) == bu.META_DTYPE and bu.META_DTYPE.itemsize == 16


def test_tile_geometry_is_the_one_the_planted_inputs_assume(skm):
    _, wave, tile = skm.fasta_parse_info()
    assert (wave, tile) == (bu.WAVE, bu.TILE)


# RULES_RECORDS = r1 (18 residues), >x (4), nobody (0), last (6)
HAND = {
    "all": (b"ACDE*FGHIKlmnpqABC\0WWWW\0\0TTTTVV\0", [0, 19, 24, 25], [18, 4, 0, 6], [0, 1, 2, 0], 11),
    "none": (b"", [], [], [], 0),
    "first": (b"ACDE*FGHIKlmnpqABC\0", [0], [18], [0], 11),
    "last": (b"TTTTVV\0", [0], [6], [0], 0),
    "alternating": (b"ACDE*FGHIKlmnpqABC\0\0", [0, 19], [18, 0], [0, 2], 11),
    "alternating_odd": (b"WWWW\0TTTTVV\0", [0, 5], [4, 6], [1, 0], 0),
}


@pytest.mark.parametrize("mask", sorted(HAND))
def test_selected_layout_of_the_rules_text(mask):
    recs = bu.records_of([fu.RULES_TEXT])
    assert recs == fu.RULES_RECORDS
    func = bu.mask_func(len(recs), mask)
    lay = bu.Layout(recs, func, base=7, first=3)
    packed, pstart, lens, funcs, windows = HAND[mask]
    assert lay.packed == packed
    assert lay.pstart.tolist() == pstart and lay.lens.tolist() == lens
    assert lay.meta["pstart"].tolist() == [p + 7 for p in pstart]
    assert lay.meta["func"].tolist() == funcs and lay.meta["len"].tolist() == lens
    assert lay.windows == windows
    assert lay.seq_id.tolist() == list(range(3, 3 + len(lens)))
    assert lay.res.tobytes() == packed.replace(b"\0", b"") and len(lay.off) == len(lens)
    withid = bu.Layout(recs, func, rec_id=[10, 20, 30, 40])
    assert withid.seq_id.tolist() == [[10, 20, 30, 40][r] for r in withid.keep.tolist()]


def test_two_files_and_an_empty_id_between_selected_records():
    """a record with an empty id is no parser record: it takes no rec_func entry, and its residues
    go nowhere even between two selected records"""
    blobs = [b">a\nACDEFGHIK\n>\nWWWW\n>b\nLMNPQRSTV", b"", b"junk\n>c x\nYY\n"]
    recs = bu.records_of(blobs)
    assert recs == [(b"a", b"ACDEFGHIK"), (b"b", b"LMNPQRSTV"), (b"c", b"YY")]
    lay = bu.Layout(recs, [1, 0, UNDEF])
    assert lay.packed == b"ACDEFGHIK\0LMNPQRSTV\0" and lay.windows == 4


def test_planted_inputs_hold_their_edges():
    T = bu.TILE
    cases = bu.planted_cases()
    facts = {k: bu.tile_facts(b, f) for k, (b, f) in cases.items()}
    for k, (recs, ev) in facts.items():
        print(k, "tiles", len(ev), "records", len(recs), "selected events per tile", ev.tolist()[:8])

    recs, ev = facts["id_at_tile_byte_0"]
    assert recs[1]["start"] == (1, 0) and recs[1]["selected"]
    print("id_at_tile_byte_0: record 1's id starts at tile 1 byte 0, its '>' is tile 0's last byte")
    recs, ev = facts["id_at_tile_byte_4095"]
    assert recs[1]["start"] == (0, T - 1) and recs[1]["res_tiles"] == (1, 1) and recs[1]["selected"]
    print("id_at_tile_byte_4095: record 1's id starts at tile 0 byte 4095")
    recs, ev = facts["body_in_next_tile"]
    assert recs[1]["start"][0] == 1 and recs[1]["res_tiles"] == (2, 2) and recs[1]["selected"]
    blob = cases["body_in_next_tile"][0]
    assert blob[2 * T - 1:2 * T + 1] == b"\nG"
    print("body_in_next_tile: record 1 starts in tile 1, its first residue is tile 2's byte 0")
    for name, sel in (("unselected_over_three_tiles", False), ("selected_over_three_tiles", True),
                      ("selected_over_three_tiles_all", True)):
        recs, ev = facts[name]
        assert recs[1]["start"][0] == 0 and recs[1]["res_tiles"] == (0, 4) and recs[1]["selected"] == sel
        assert recs[0]["start"][0] == 0 and recs[2]["start"][0] == 4  # tiles 1, 2, 3 hold nothing else
        if name == "unselected_over_three_tiles":
            assert recs[0]["selected"] and recs[2]["selected"] and ev[1:4].tolist() == [0, 0, 0] and ev[0] and ev[4]
        elif name == "selected_over_three_tiles":
            assert not recs[0]["selected"] and not recs[2]["selected"] and ev.sum() == 4 * T + 1
            assert min(ev[1:4]) > 4000  # whole tiles of residues (less the newlines)
        print(name + ": record 1 starts in tile 0 and its residues span tiles 0..4")
    for m in ("all", "none", "alternating", "alternating_odd"):
        recs, ev = facts["tile_of_starts_" + m]
        blob = cases["tile_of_starts_" + m][0]
        assert blob[T:2 * T] == b">a\n\n" * 1024
        in_tile = [r for r in recs if r["start"][0] == 1]
        assert len(in_tile) == 1024 and all(r["res_tiles"] is None for r in in_tile)
        assert ev[1] == {"all": 1024, "none": 0, "alternating": 512, "alternating_odd": 512}[m]
        assert recs[1025]["start"] == (2, 1) and recs[1025]["res_tiles"] == (2, 2)
        print("tile_of_starts_" + m + ": tile 1 holds 1024 record starts and nothing else,", int(ev[1]), "selected")
    for name, want in (("tile_of_gt_a_nl_all", 683 + 682), ("tile_of_gt_a_nl_alternating", 341 + 341),
                       ("tile_of_gt_a_nl_none", 0), ("tile_of_gt_a_nl_none_at_all", 0)):
        recs, ev = facts[name]
        assert cases[name][0][T:2 * T] == b">a\n" * 1365 + b">"
        in_tile = [r for r in recs if r["start"][0] == 1]
        assert len(recs) == 685 and len(in_tile) == 683 and in_tile[0]["start"] == (1, 1)
        assert in_tile[-1]["res_tiles"] == (2, 2) and all(r["res_tiles"] == (1, 1) for r in in_tile[:-1])
        assert ev[1] == want
        if name == "tile_of_gt_a_nl_none":  # output before and after the silent tile
            assert ev[0] == 14 and ev[2] == 17 and not any(r["selected"] for r in in_tile)
        if name == "tile_of_gt_a_nl_none_at_all":
            assert ev.sum() == 0
        print(name + ": tile 1 holds 683 record starts and 682 residues;", int(ev[1]), "selected events")
    for name in ("unwrapped_line_selected", "unwrapped_line_all"):
        recs, ev = facts[name]
        assert ev[1] == T and ev[2] == T and recs[1]["res_tiles"] == (0, 3)
        print(name + ": tiles 1 and 2 put out 4096 bytes each")
    recs, ev = facts["empty_tile_between"]
    assert ev[1] == 0 and ev[0] > 0 and ev[2] > 0 and not recs[1]["selected"] and recs[1]["res_tiles"] == (0, 2)
    print("empty_tile_between: tile 1 has no selected event, tiles 0 and 2 have", int(ev[0]), int(ev[2]))
