"""The chunk scan (k_scan_blocks, rio_chunk_scan.hip) and the placement prologue (k_place, rio_place.hip) at the
boundaries of the scan tree. At 64-byte chunks a level-1 block is 16 KiB of file, level 2 runs in one wave up to
1 MiB and in tiles with a carry beyond, the second tile from 4 MiB on: the files of tests/scan_cases.py put
clean ends, terminal statuses, broken entries on the chain, span ends, truncations and zero tails at the first
and last chunk of a block, of the 64-block switch and of a tile, under the wave walk and the lane walk.

Every decode must equal the oracle's (oracle_py.file_reader_decode_arrays) bit for bit, report the chunk count
the case was built for (so the intended tree was reached and the chunk size honoured), and report exactly the
repairs the sequential model counts from the file's ledger (scan_cases.model). That count shows a break the scan
misses (0 where an entry on the chain is wrong) and a repair that walks the wrong chunks. It does not show the
path taken: slow_path counts only entered chunks whose entry is not where the chain arrives, so a run that
breaks spuriously on a clean file reports 0 like the fast path, and ScanState::slow is not in rio_file_info.
tests/test_scan_cases_host.py holds the same list to the oracle without a GPU.

Test ids: N<chunks> for the shapes; <tree>-c<chunk>-<kind> for the events (trees N1 = 600 chunks, level 2 in one
wave; N2 = 16 984, one tile; N3 = 66 136, two tiles); span<A|B|C> for the spans."""
import functools

import pytest

import oracle_py as orc
import scan_cases as SC
from gpu_util import assert_same_as_oracle, decode_with, decoder_with_env

pytestmark = pytest.mark.gpu

WAVE64 = {"RIO_WALK_LANE": "0", "RIO_CHUNK_BYTES": "64"}
LANE64 = {"RIO_WALK_LANE": "1", "RIO_LANE_CHUNK_BYTES": "64"}
# the topmost parametrisation varies fastest: a group's files are decoded under both walks while they are cached
framings = pytest.mark.parametrize("env", [pytest.param(WAVE64, id="wave64"), pytest.param(LANE64, id="lane64")])

SHAPES = [g for g in SC.GROUPS if "-" not in g and g.startswith("N")]
EVENTS = [g for g in SC.GROUPS if g[:3] in ("N1-", "N2-", "N3-")]
SPANS = [g for g in SC.GROUPS if g.startswith("span") and g != "span_with_false_entries" or g == "one-record"]
assert len(SHAPES) + len(EVENTS) + len(SPANS) + 1 == len(SC.GROUPS)


@functools.lru_cache(maxsize=24)
def oracle(case_id: str) -> dict:
    """The oracle's decode of a case, computed once and left unchanged."""
    return orc.file_reader_decode_arrays(SC.built(case_id)[0])


def check(dec, case_id: str):
    img, led, m = SC.built(case_id)
    o = oracle(case_id)
    g = decode_with(dec, img)
    assert_same_as_oracle(g, o, case_id)
    assert g["n_chunks"] == m["n_chunks"] == SC.BY_ID[case_id].n_chunks, (case_id, g["n_chunks"], m["n_chunks"])
    print(f"{case_id}: n_chunks {g['n_chunks']} n_repairs {g['n_repairs']} expected {m['expected_repairs']}"
          f" must_be_fast {m['must_be_fast']}")
    assert g["n_repairs"] == m["expected_repairs"], (case_id, g["n_repairs"], m["expected_repairs"])
    return g


def check_group(group, env, monkeypatch):
    dec = decoder_with_env(monkeypatch, env)
    for case in SC.GROUPS[group]:
        check(dec, case.id)


@framings
@pytest.mark.parametrize("group", SHAPES)
def test_shape(group, env, monkeypatch):
    """Clean files of N chunks, the last one full and again one byte long: records that start every chunk, that drift
    through the chunks, and that leave chunks without a record start (a run whose key is kNone)."""
    for case in SC.GROUPS[group]:
        assert SC.built(case.id)[2]["must_be_fast"] or case.id.startswith("shape-N1-") and case.id.endswith("last1")
    check_group(group, env, monkeypatch)


@framings
@pytest.mark.parametrize("group", EVENTS)
def test_event(group, env, monkeypatch):
    """One event in chunk c of a tree: a wrong header CRC behind its chunk's first record (fast path), in it (the
    speculative entry is a later record, or none: repaired), a file that ends inside a header or a payload, a zero
    tail from the middle of the chunk or from its first byte, a valid record inside a payload right where a chunk
    begins (one repair)."""
    check_group(group, env, monkeypatch)


@framings
@pytest.mark.parametrize("group", SPANS)
def test_span(group, env, monkeypatch):
    """One record over whole blocks (span A: blocks 1 and 2 own nothing and the next record opens block 3, or starts
    1 or 63 bytes into it, or the file ends with the span), over the 64 blocks of the one-wave switch (B), over a
    whole tile whose block runs meet the carry (C), or over the whole file."""
    check_group(group, env, monkeypatch)


@framings
def test_span_with_false_entries(env, monkeypatch):
    """Spans A and C with runs of valid records inside the payload: at a block's first byte, across a block
    boundary, across the tile boundary. No chunk the chain enters has a wrong entry, so the count is 0 whether the
    composed run breaks on the false runs or passes over them."""
    for case in SC.GROUPS["span_with_false_entries"]:
        m = SC.built(case.id)[2]
        assert m["expected_repairs"] == 0 and not m["must_be_fast"]
    check_group("span_with_false_entries", env, monkeypatch)


@framings
def test_one_context_many_files(env, monkeypatch):
    """Larger and smaller files, fast and repaired, through one context with nothing recreated in between: block runs
    and chunk prefixes a larger predecessor left in the arena must not reach a smaller file, and the arrival ticket
    starts from zero each time."""
    dec = decoder_with_env(monkeypatch, env)
    seen = [check(dec, case_id)["n_repairs"] for case_id in SC.ONE_CONTEXT]
    assert seen[0] == 0 and seen[2] >= 1 and seen[6] == 1 and seen[7] == 0, seen
