"""The four-buffer int8 scan bodies (tools/gen_scan_asm.py, generate(..., qbufs=4)): an image of six 32 KiB chunks, chunk c in
LDS buffer c & 3, chunks 2 and 3 written once per launch, two chunks staged per tile.  CPU only: the schedule is a pure
function and the bodies are text -- the scalar address arithmetic of that text is replayed here, instruction by
instruction, for one wave over four tiles."""
import hashlib
import importlib.util
import re
from collections import defaultdict
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SPACES = ["cosine", "l2", "ip"]
NKC = 6
CHUNK = 0x8000

# sha256 of generate(space, 4, i8=True, nqt=nqt, l2c=space == "l2") at the commit before the four-buffer bodies: the
# default (two-buffer) bodies must not change by a byte
PINNED = {
    ("cosine", 16): "24420fc7afe0f2739ea37e415a86d9aae7f24bd28f723593c9676c1abffac929",
    ("cosine", 8): "8e462ce81b75b86431d6e73d3342d4e4b711d39b1cdd464ff88239c7a627e258",
    ("cosine", 4): "48228e24b3e4453d676ca19fe5882b2f0345184c7c3366fbd0477f3ab688f489",
    ("l2", 16): "279e861ab05f62a4905f083120ccd8e153ce494604c88048002d37d39183e208",
    ("l2", 8): "0dfb2064e19baba27a3f0625790d5d408f8d9b53483019254b97f8ba586e58bd",
    ("l2", 4): "7f3773e108b508a14d1b9db300288ee7db16c01b6f2a5a104308fbc66a73a7dd",
    ("ip", 16): "bb6b2b3826db9523bc7c9d087334eb541b6a272df81cd3bd9d6cfcb0d8104ad6",
    ("ip", 8): "7ed0eac14b9ea3be55fda1d1e1aeff0069dcf7bc52cfecd9cd595e7b7c1adc4b",
    ("ip", 4): "26ea754205bd9cfce3b10463f1f0cf4004958517d6fc3b7f80bbf9d11a6e2615",
}


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_qbufs4", ROOT / "tools" / "gen_scan_asm.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def code_lines(body):
    return re.findall(r'^\s+"(.*?)\\n\\t"$', body, flags=re.M)


def section(lines, start, end):
    return lines[lines.index(start) + 1: lines.index(end)]


def q4_text(gen, space, sparse):
    gen.Q4_SPARSE_BARRIERS = sparse
    return gen.generate(space, 4, i8=True, nqt=16, l2c=space == "l2", qbufs=4)


# ------------------------------------------------------------------------------------------------ the schedule
def test_schedule_of_four_buffers_over_four_consecutive_tiles():
    """Walk q_schedule(6, 4) the way a workgroup does: prologue, then tiles of parity 0, 1, 0, 1."""
    table = load_generator().q_schedule(NKC, 4)
    assert len(table) == 2 and all(len(rows) == NKC for rows in table)
    held = {c: c for c in range(4)}      # buffer -> chunk: what the prologue stages
    uses = [table[t & 1][p][0] for t in range(4) for p in range(NKC)]
    for t in range(4):
        rows = table[t & 1]
        chunks = [r[0] for r in rows]
        assert chunks == (list(range(NKC)) if t & 1 == 0 else list(range(NKC - 1, -1, -1))), "even tiles ascend, odd descend"
        assert [r[2] is not None for r in rows] == [False, False, False, True, True, False]
        staged = 0
        for p, (chunk, buf, stage) in enumerate(rows):
            assert buf == chunk & 3
            assert held[buf] == chunk, f"tile {t} position {p}: chunk {chunk} is not resident in buffer {buf}: {held}"
            if stage is not None:
                s_chunk, s_buf = stage
                assert s_buf in (0, 1), "buffers 2 and 3 are never written after the prologue"
                assert s_buf != buf, "the current buffer is never written"
                assert s_chunk == uses[t * NKC + p + 1], "prefetch distance is one chunk"
                held[s_buf] = s_chunk
                staged += 1
        assert staged == 2, f"tile {t} stages {staged} chunks"
        assert held[2] == 2 and held[3] == 3


def test_stage_and_barrier_flags_per_body():
    gen = load_generator()
    assert gen.body_stage_flags(4) == {"first": (False, False), "mid": (False, True), "last": (True, False)}
    assert gen.q4_barrier_flags(False) == {"first": (True, True), "mid": (True, True), "last": (True, True)}
    assert gen.q4_barrier_flags(True) == {"first": (False, True), "mid": (False, True), "last": (True, False)}
    assert gen.lds_stage_cap(2) == 992 and gen.lds_stage_cap(4) == 304
    assert 4 * CHUNK + 3072 + 8 * 12 * gen.lds_stage_cap(4) <= 160 * 1024
    # the earlier schedules keep their results
    assert gen.body_stage_flags(2) == {"single": (False, False), "first": (False, True), "mid": (True, True), "last": (True, False)}
    assert gen.body_stage_flags(3)["first"] == (False, False)


# ------------------------------------------------------------------------------------------------ the text
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("space", SPACES)
def test_body_text(space, sparse):
    gen = load_generator()
    body = q4_text(gen, space, sparse)
    assert body.count("asm volatile(") == 1
    lines = code_lines(body)
    tile = section(lines, ".Ltile_%=:", "s_cbranch_scc1 .Ltile_%=")
    # the direction lives in two SGPRs, uniform over the workgroup: the tile loop holds no branch on it
    for i, ln in enumerate(tile):
        if ln.startswith("s_cmp") and (gen.XSTEP in ln or gen.QSTEP in ln):
            assert tile[i + 1].startswith("s_cselect"), f"a branch on the tile's direction: {tile[i + 1]}"
    first = section(lines, ".Ltile_%=:", ".Lloop_%=:")
    mid = section(lines, "s_cbranch_scc1 .Llast_%=", "s_branch .Lloop_%=")
    last = section(lines, ".Llast_%=:", ".Ladmit_%=:")
    assert ".Lsingle_%=:" not in lines, "a tile of six chunks is three bodies"
    pieces = len(gen.dma_pieces())
    assert pieces == 4
    for name, part in (("first", first), ("mid", mid), ("last", last)):
        assert sum("offen lds" in ln for ln in part) == pieces * sum(gen.body_stage_flags(4)[name]), name
        assert part.count("s_barrier") == sum(gen.q4_barrier_flags(sparse)[name]), name
        # the read base moves at every position but a tile's first, by the direction register, and wraps at 128 KiB
        moves = [i for i, ln in enumerate(part) if ln == f"v_add_u32 %[ldr], {gen.QSTEP}, %[ldr]"]
        assert len(moves) == (1 if name == "first" else 2), name
        assert all(part[i + 1] == "v_and_b32 %[ldr], 0x1ffff, %[ldr]" for i in moves)
        assert not any("v_xor_b32 %[ldr]" in ln for ln in part)
    # every barrier sits in straight-line code: none out of line (hit stubs, append routine), none between a branch on VCC
    # or EXEC and its target
    end = lines.index("s_branch .Ldone_%=")
    assert "s_barrier" not in lines[end:]
    for i, ln in enumerate(lines[:end]):
        m = re.match(r"s_cbranch_(vcc|exec)\w* (\S+)", ln)
        if m:
            target = lines.index(m.group(2) + ":")
            assert target > end or "s_barrier" not in lines[min(i, target):max(i, target)], ln
    if sparse:   # nothing follows a tile's last reads: the barrier that frees the Q buffers for the wrapper's tail
        assert lines[end - 2:end] == ["s_waitcnt vmcnt(0) lgkmcnt(0)", "s_barrier"]


# ------------------------------------------------------------------------------------------------ the replay
class Replay:
    """One wave's walk through a body: the scalar instructions (and the three VALU ones that move the read base) are executed,
    reads of the Q buffers, transfers into them, vmcnt waits and barriers are recorded with the barrier epoch they fall in.
    All eight waves run this same instruction sequence, and between two barriers each is free to be anywhere: an event of one
    wave is known to precede an event of another only if a barrier lies between them in program order (epoch a < epoch b)."""

    def __init__(self, lines, ntiles):
        self.lines = lines
        self.labels = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
        self.r = defaultdict(int)
        self.r.update({"%[qbytes]": NKC * CHUNK, "%[nb]": NKC // 2, "%[ntiles]": ntiles, "%[pb]": 768 * 16, "%[wave2k]": 3 * 2048,
                       "%[qvoff]": 3 * 2048 + 5 * 16, "%[lane16]": 5 * 16})
        self.scc = 0
        self.epoch = 0
        self.vm = []          # in-order queue: [kind, payload, done_epoch or None]
        self.events = []      # ("read", buffer, epoch) / ("write", buffer, chunk, epoch, op)

    def val(self, tok):
        tok = tok.strip()
        if re.fullmatch(r"-?(0x[0-9a-f]+|\d+)", tok):
            return int(tok, 0) & 0xffffffff
        return self.r[tok]

    def run(self):
        pc = 0
        while True:
            ln = self.lines[pc]
            pc += 1
            if ln.endswith(":"):
                continue
            op, _, rest = ln.partition(" ")
            a = [x.strip() for x in rest.split(",")]
            if op == "s_branch":
                if a[0] == ".Ldone_%=":
                    return self
                pc = self.labels[a[0]]
            elif op in ("s_cbranch_scc0", "s_cbranch_scc1"):
                if self.scc == (op[-1] == "1"):
                    pc = self.labels[a[0]]
            elif op.startswith("s_cbranch_"):
                pass                                            # admission pre-tests: nothing passes in this replay
            elif op in ("s_mov_b32", "s_movk_i32", "v_mov_b32"):
                self.r[a[0]] = self.val(a[1])
            elif op in ("s_add_u32", "v_add_u32"):
                t = self.val(a[1]) + self.val(a[2])
                self.r[a[0]] = t & 0xffffffff
                if op[0] == "s":
                    self.scc = t >> 32
            elif op == "s_sub_u32":
                t = self.val(a[1]) - self.val(a[2])
                self.r[a[0]], self.scc = t & 0xffffffff, int(t < 0)
            elif op in ("s_xor_b32", "v_xor_b32"):
                self.r[a[0]] = self.val(a[1]) ^ self.val(a[2])
            elif op == "v_and_b32":
                self.r[a[0]] = self.val(a[1]) & self.val(a[2])
            elif op == "s_lshr_b32":
                self.r[a[0]] = self.val(a[1]) >> self.val(a[2])
            elif op == "s_cmp_eq_u32":
                self.scc = int(self.val(a[0]) == self.val(a[1]))
            elif op == "s_cmp_lg_u32":
                self.scc = int(self.val(a[0]) != self.val(a[1]))
            elif op == "s_cmp_gt_u32":
                self.scc = int(self.val(a[0]) > self.val(a[1]))
            elif op == "s_cmp_gt_i32":
                sg = lambda v: v - (1 << 32) if v >> 31 else v
                self.scc = int(sg(self.val(a[0])) > sg(self.val(a[1])))
            elif op == "s_cselect_b32":
                self.r[a[0]] = self.val(a[1]) if self.scc else self.val(a[2])
            elif op == "s_barrier":
                self.epoch += 1
            elif op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", rest)
                if m:
                    n = int(m.group(1))
                    for e in self.vm[:len(self.vm) - n]:
                        if e[2] is None:
                            e[2] = self.epoch
            elif op == "ds_read_b128" and a[1].startswith("%[ldr]"):
                off = int(re.search(r"offset:(\d+)", ln).group(1))
                assert off < CHUNK
                self.events.append(("read", self.val("%[ldr]") // CHUNK, self.epoch))
            elif op.startswith("buffer_load") or op.startswith("global_"):
                e = ["x", None, None]
                if "%[qsrd]" in ln:
                    src = self.val("%[qvoff]") + self.val(a[-1].split()[0])   # offen: VGPR offset + soffset
                    assert src < NKC * CHUNK
                    assert ln.endswith("offen lds"), "the query image reaches LDS by LDS-DMA only"
                    dst = self.val("m0") + self.val("%[lane16]")
                    assert dst % CHUNK == src % CHUNK, "a piece keeps its place inside the chunk"
                    e = ["q", src, None]
                    self.events.append(("write", dst // CHUNK, src // CHUNK, self.epoch, e))
                self.vm.append(e)


def check_rules(events, bufs, ntiles):
    """Residency and order of every chunk position, and the two barrier rules for every transfer and every first read."""
    held = {}                 # buffer -> (chunk, the write events that brought it)
    last_read = {}            # buffer -> epoch of the last read so far
    reads_seen = []
    for ev in events:
        if ev[0] == "write":
            _, buf, chunk, epoch, op = ev
            assert 0 <= buf < bufs
            # rule 1: every wave's last read of what the buffer held lies behind a barrier
            assert buf not in last_read or last_read[buf] < epoch, f"transfer of chunk {chunk} into buffer {buf} may overtake a read"
            if buf in held and held[buf][0] == chunk:
                held[buf][1].append(op)
            else:
                held[buf] = (chunk, [op])
                if reads_seen:
                    assert buf in (0, 1), "buffers 2 and 3 are never written after the prologue"
        else:
            _, buf, epoch = ev
            chunk, ops = held[buf]
            # rule 2: this wave waited for its pieces, and a barrier lies between that wait and this read
            for op in ops:
                assert op[2] is not None and op[2] < epoch, f"chunk {chunk} in buffer {buf} read before its transfer is published"
            last_read[buf] = epoch
            reads_seen.append(chunk)
    per_pos = 2 * 16          # B fragments per chunk position
    want = [c for t in range(ntiles) for c in (range(NKC) if t & 1 == 0 else range(NKC - 1, -1, -1)) for _ in range(per_pos)]
    assert reads_seen == want, "every position reads the chunk of its place in the zig-zag order"
    return held


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("space", SPACES)
def test_replay_of_four_tiles_keeps_the_barrier_rules(space, sparse):
    gen = load_generator()
    lines = code_lines(q4_text(gen, space, sparse))
    rp = Replay(lines, 4).run()
    writes = [e for e in rp.events if e[0] == "write"]
    pieces = len(gen.dma_pieces())
    assert len(writes) == pieces * (4 + 2 * 4), "the prologue stages four chunks, every tile two"
    assert all(e[1] in (0, 1) for e in writes[4 * pieces:])
    held = check_rules(rp.events, 4, 4)
    assert held[2][0] == 2 and held[3][0] == 3
    assert rp.epoch == 1 + 4 * (3 if sparse else 6) + (1 if sparse else 0)


@pytest.mark.parametrize("space", SPACES)
def test_the_replay_also_accepts_the_two_buffer_body(space):
    """The model is not made to fit the new bodies: the default body, on the same six-chunk image, passes it too."""
    gen = load_generator()
    lines = code_lines(gen.default_i8_body(space))
    rp = Replay(lines, 4).run()
    check_rules(rp.events, 2, 4)
    assert sum(e[0] == "write" for e in rp.events) == len(gen.dma_pieces()) * (2 + 4 * 4)


def test_the_replay_rejects_a_missing_barrier():
    """Take the barrier after position 3 out of the sparse body: the chunk staged there is then read unpublished."""
    gen = load_generator()
    lines = code_lines(q4_text(gen, "cosine", True))
    mid_end = lines.index("s_branch .Lloop_%=")
    k = max(i for i in range(mid_end) if lines[i] == "s_barrier")
    with pytest.raises(AssertionError, match="published"):
        check_rules(Replay(lines[:k] + lines[k + 1:], 4).run().events, 4, 4)


# ------------------------------------------------------------------------------------------------ the default bodies
def test_default_bodies_are_unchanged():
    gen = load_generator()
    texts = {}
    for (space, nqt), digest in PINNED.items():
        text = gen.generate(space, 4, i8=True, nqt=nqt, l2c=space == "l2")
        assert text == gen.generate(space, 4, i8=True, nqt=nqt, l2c=space == "l2", qbufs=2)
        assert hashlib.sha256(text.encode()).hexdigest() == digest, (space, nqt)
        texts[(space, nqt)] = text
    q4_text(gen, "cosine", True)   # generating a four-buffer body leaves no state behind
    for (space, nqt), text in texts.items():
        assert gen.generate(space, 4, i8=True, nqt=nqt, l2c=space == "l2") == text
    assert len(set(texts.values())) == 9


# ------------------------------------------------------------------------------------------------ the dispatch
def test_only_knn_passes_of_small_k_ask_for_the_four_buffer_body():
    """The small staging area is safe for k <= 64 kNN passes only: the flag is set in run_filter_pass and nowhere else, and
    launch_scan_space asks for it, a full pass and the six-chunk image before it takes the body."""
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    api = (csrc / "api.hip").read_text()
    sets = [m.start() for m in re.finditer(r"\bscan_q4\s*=[^=]", api)]
    assert len(sets) == 1
    a, b = api.index("int run_filter_pass("), api.index("int attach_mid(")
    assert a < sets[0] < b and "fa.scan_q4 = k <= 64;" in api[a:b]
    for other in csrc.glob("*.hip"):
        if other.name != "api.hip":
            assert not re.search(r"\bscan_q4\s*=[^=]", other.read_text()), other.name
    filt = (csrc / "kernels_filter.hip").read_text()
    assert "if (a.scan_q4 && a.nq > 128 && a.ld8 == kAsmQ4Chunks * 2 * kFilterChunkK)" in filt
    assert filt.count("launch_scan_asm<SPACE, 4, true, 16, 4>") == 1
    # what bench.py's source hash slices the wrapper by
    assert filt.index("void filter_scan_asm_kernel(") < filt.index(
        "// ------------------------------------------------------------------ threshold update + compaction")
