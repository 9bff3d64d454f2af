"""The zig-zag order of the int8 scan's k-chunks (tools/gen_scan_asm.py, q_schedule): a workgroup's even tiles walk the
chunks of the query image upwards, its odd tiles downwards, so the chunks a tile ends on are still in LDS when the next
tile starts on them.  CPU only: the schedule is a pure function, the bodies are text."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_zigzag", ROOT / "tools" / "gen_scan_asm.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.mark.parametrize("bufs", [2, 3])
@pytest.mark.parametrize("nkc", [2, 4, 6, 8, 16])
def test_schedule_over_four_consecutive_tiles(nkc, bufs):
    """Walk q_schedule the way a workgroup does: prologue, then tiles of parity 0, 1, 0, 1."""
    table = load_generator().q_schedule(nkc, bufs)
    assert len(table) == 2 and all(len(rows) == nkc for rows in table)
    held = {c % bufs: c for c in range(min(nkc, bufs))}      # buffer -> chunk: what the prologue stages
    assert len(held) == min(nkc, bufs)
    # position (tile-major) of every use of a chunk, to know the last use of what a buffer holds
    uses = [(t, p, table[t & 1][p][0]) for t in range(4) for p in range(nkc)]
    stagings = []
    for t in range(4):
        rows = table[t & 1]
        chunks = [r[0] for r in rows]
        assert sorted(chunks) == list(range(nkc)), "a tile uses every chunk exactly once"
        assert chunks == (list(range(nkc)) if t & 1 == 0 else list(range(nkc - 1, -1, -1))), "even tiles ascend, odd descend"
        n_staged = 0
        for p, (chunk, buf, stage) in enumerate(rows):
            assert 0 <= buf < bufs
            assert held.get(buf) == chunk, f"tile {t} position {p}: chunk {chunk} is not resident in buffer {buf}: {held}"
            if stage is not None:
                s_chunk, s_buf = stage
                assert 0 <= s_chunk < nkc and 0 <= s_buf < bufs
                assert s_buf != buf, "the current buffer is never written"
                nxt = uses[t * nkc + p + 1][2] if t * nkc + p + 1 < len(uses) else None
                assert nxt is None or s_chunk == nxt, "prefetch distance is one chunk"
                # (overwriting a chunk before its last read would fail the residency check at that read: `held` is the
                # buffers' true content over the four tiles)
                held[s_buf] = s_chunk
                n_staged += 1
        stagings.append(n_staged)
    want = max(0, nkc - bufs) if nkc > bufs else 0
    assert stagings == [want] * 4, f"stagings per tile {stagings}, want {want} (the prologue makes the first tile a steady-state one)"


@pytest.mark.parametrize("bufs", [2, 3])
def test_staging_positions_depend_on_the_body_alone(bufs):
    """The bodies are generic over nkc and the direction: first / middle / last / single body each stage at fixed positions."""
    flags = load_generator().body_stage_flags(bufs)
    assert flags["single"] == (False, False) and flags["mid"] == (True, True) and flags["last"] == (True, False)
    assert flags["first"] == ((False, True) if bufs == 2 else (False, False))


def code_lines(body):
    return re.findall(r'^\s+"(.*?)\\n\\t"$', body, flags=re.M)


def section(lines, start, end):
    return lines[lines.index(start) + 1: lines.index(end)]


@pytest.mark.parametrize("nqt", [16, 8, 4])
@pytest.mark.parametrize("space", ["cosine", "ip", "l2"])
def test_every_int8_body_generates_with_one_barrier_per_chunk_in_both_directions(space, nqt):
    gen = load_generator()
    body = gen.generate(space, 4, i8=True, nqt=nqt, l2c=space == "l2")
    assert body.count("asm volatile(") == 1
    lines = code_lines(body)
    tile = section(lines, ".Ltile_%=:", "s_cbranch_scc1 .Ltile_%=")
    # Both directions run the same instructions -- the direction lives in two SGPRs (the X cursors' step, the Q cursor's
    # step), uniform over the workgroup -- so the forward and the reverse path cannot differ in barriers: the tile loop
    # holds no branch on the direction, and one s_barrier per chunk of each of its four bodies.
    xstep, qstep = gen.XSTEP, gen.QSTEP
    for i, ln in enumerate(tile):
        if ln.startswith("s_cmp") and (xstep in ln or qstep in ln):
            assert tile[i + 1].startswith("s_cselect"), f"a branch on the tile's direction: {tile[i + 1]}"
    first = section(lines, "s_cbranch_scc1 .Lsingle_%=", ".Lloop_%=:")
    mid = section(lines, "s_cbranch_scc1 .Llast_%=", "s_branch .Lloop_%=")
    last = section(lines, ".Llast_%=:", "s_branch .Ladmit_%=")
    single = section(lines, ".Lsingle_%=:", ".Ladmit_%=:")
    for name, part in (("first", first), ("mid", mid), ("last", last), ("single", single)):
        assert part.count("s_barrier") == 2, name
        # a position that stages nothing issues no transfer, and the toggle is skipped exactly at a tile's first chunk
        flags = gen.body_stage_flags(2)[name]
        assert sum("offen lds" in ln for ln in part) == len(gen.dma_pieces()) * sum(flags), name
        assert sum(ln.startswith("s_xor_b32 %[sldw]") for ln in part) == (1 if name in ("first", "single") else 2), name


def test_bf16_bodies_keep_the_ascending_schedule():
    gen = load_generator()
    body = gen.generate("cosine", 4)
    lines = code_lines(body)
    assert "s_mov_b32 %[qcur], %[qc1]" in lines and gen.XSTEP not in body and gen.QSTEP not in body
    assert sum("offen lds" in ln for ln in lines) == 4 + 4 * 2 * 4   # prologue + every chunk of the four bodies stages
