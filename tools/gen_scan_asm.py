#!/usr/bin/env python3
"""Generates the gfx950 assembly of the filter scan (MFMA bounds of all rows x 256 queries).

Output: mlvectordb_amd/csrc/scan_asm_*.inc -- ONE `asm volatile(...)` statement per body, the whole body of
filter_scan_asm_kernel (kernels_filter.hip): prologue, the persistent loop over the workgroup's row tiles, the k-loop of a
tile, the admission test and the (rare) append path.  The bodies (entries() below): the bf16 body per space and ring depth,
and the int8 body per space and query-tile count.

Why assembly: hipcc's schedule of the same loop drains the X prefetch every two k-steps
(vmcnt(0) + register copies at the back edge), reads each B fragment right before its MFMAs, and
spills around the epilogue; values that are the targets of loads still in flight cannot be handed
through compiler-managed code at all.  Here everything that is in flight stays inside one
statement, and the waits are computed by simulating the two in-order queues (vmcnt: buffer/global
operations; lgkmcnt: LDS operations).

Per wave: MT = 2 row panels (16 rows each) x 16 query tiles = 32 accumulators of 16x16, two waves per SIMD, 8 waves per
workgroup.  bf16 bodies: hipcc splits the 256 registers 128 VGPR / 128 AGPR as soon as a kernel touches an AGPR, so the
accumulators take the AGPRs (a[0:127]) and everything else lives in <= 128 VGPRs.  int8 bodies: the accumulators are
ArchVGPRs (see generate).
  * X (shadow panels, HBM): buffer_load_dwordx4 into a ring of R k-steps that are the MFMA A
    operands; a slot is refilled right after its last MFMA with the k-step R ahead -- the last R
    k-steps of a tile fetch the first R of the workgroup's next tile through a second descriptor,
    so the stream never stops, not even during the admission test.  Streamed once: non-temporal.
  * Q (query image, L2): 64-column chunks, double buffered in LDS, one s_barrier per chunk.  Early
    in chunk c every wave sends its share of chunk c+1 global -> LDS directly (buffer_load ... lds;
    the LDS address is M0 + 16*lane) and waits for it before the barrier.  vmcnt completes in
    order, so waiting for a Q transfer also waits for every X refill issued before it.  The int8 bodies (integer sums: any
    chunk order gives the same bits) walk the chunks zig-zag, up in a workgroup's even tiles and down in its odd ones, and
    stage only the chunks that are not still in LDS from the turn (q_schedule).  An image of exactly six chunks (ld8 = 768)
    also has bodies with FOUR buffers (generate(..., qbufs=4)): chunks 2 and 3 stay in LDS for the whole launch, a tile
    stages two chunks instead of four, and the wave's append staging area shrinks to what is left.
  * the 32 B fragments of a chunk are one software-pipelined stream: ds_read_b128 runs QD
    fragments ahead of the two MFMAs that consume a fragment.
  * admission test per query tile: 8 bounds per lane (same arithmetic as scan_epilogue), their
    maximum against the threshold; only if some lane passes, an out-of-line routine appends
    (bound, row, query) entries to the WAVE's private buffer, staged in LDS until the kernel ends:
    the fill count lives in an SGPR, slots come from v_mbcnt -- no atomic, no wait, and no global
    store in the loop (see gen_slow).  The kernel's C++ tail then moves the entries into the
    per-query lists.  The routine's memory
    operations are younger than every prefetch, so the counted waits elsewhere stay sufficient.
"""
import argparse
from pathlib import Path

MT = 2                    # row panels of 16 rows per wave
NW = 8                    # waves per workgroup
QD = 4                    # B fragments read ahead of their MFMAs
CHUNK_BYTES = 0x8000      # 256 queries x 64 columns x 2 B
Q_BUFS = 2                # Q chunk buffers in LDS (kAsmQBufs: scan_asm_consts.inc)
WG_CAP = 16384            # kWgCap: append entries per workgroup (split evenly over its waves)
SPACES = {"l2": 0, "cosine": 1, "ip": 2}
I8_SPACE = None
I8 = False     # generate(): int8 shadow -- v_mfma_i32_16x16x64_i8, k-steps of 64 columns, integer accumulators in ArchVGPRs
#                v[VA_BASE : VA_BASE + 64*MT), the admission test folded into the tile's last k-step (see generate)
VA_BASE = 64   # v0..v63 stay with the compiler (the statement's "v" operands)
L2C = False    # generate(): int8 l2 -- the admission test made sharp by per-row integer offsets that enter the accumulators
#                through the first k-step's C operand, ONE query scale SQ and ONE error coefficient KE for the whole pass (the
#                prep builds the images that way): the pre-test is cosine's -- one fma against a threshold held in a register
ZZ = False     # generate(): the int8 bodies walk the k-chunks zig-zag -- up in a workgroup's even tiles, down in its odd ones (q_schedule)
QB = 2         # generate(): Q chunk buffers of the body being generated: 2, or 4 (int8, NQT = 16, nkc = 6 only: chunks 2 and 3 stay in
#                buffers 2 and 3 for the whole launch, a tile stages two chunks instead of four; see generate)
Q4_NKC = 6     # the only chunk count the four-buffer bodies are written for (ld8 = 768)
Q4_SPARSE_BARRIERS = False   # four-buffer bodies: False = one s_barrier per chunk position; True = only the barriers the two rules
#                of q4_barrier_flags need (measured: DESIGN 5.2)
NQT = 16       # generate(): query tiles (of 16 queries) the body computes: 16 = a full 256-query pass; 8 / 4 (int8 bodies) for
#                passes of <= 128 / <= 64 queries -- the MFMAs, B-fragment reads, Q staging and admission tests of the empty tiles are
#                not issued at all, which leaves a pure stream of the shadow (see generate)


class VmWait:
    """A counted vmcnt wait site in Sched.lines: n operations may stay in flight (None: an earlier wait covers it).  What
    was issued before a body depends on which body ran before it; body_lines simulates every predecessor sequence and
    keeps, per site, the smallest count."""

    def __init__(self, n):
        self.n = n


def merge_waits(variants):
    """Line lists of one body under different histories -> one list; every VmWait site takes its strictest count."""
    assert len({len(v) for v in variants}) == 1
    out = []
    for group in zip(*variants):
        if isinstance(group[0], VmWait):
            counts = [w.n for w in group if w.n is not None]
            if counts:
                out.append(f"s_waitcnt vmcnt({min(counts)})")
        else:
            assert all(g == group[0] for g in group), group
            out.append(group[0])
    return out


class Sched:
    """Instruction list + in-order queue simulation for counted waits."""

    def __init__(self):
        self.lines = []
        self.vm = []
        self.lg = []
        self.vm_done = 0
        self.lg_done = 0
        self.recording = True
        self.label = 0
        self.copy = ""   # which copy of the tile's last body this is (int8: its hit stubs return into it)

    def emit(self, text):
        if self.recording:
            self.lines.append(text)

    def vmem(self, text, tag):
        self.emit(text)
        self.vm.append(tag)

    def lds(self, text, tag):
        self.emit(text)
        self.lg.append(tag)

    def _last(self, q, tag):
        for i in range(len(q) - 1, -1, -1):
            if q[i] == tag:
                return i
        if not self.recording:
            return -1      # warm-up pass: nothing older exists yet
        raise KeyError(tag)

    def need_vm(self, *tags):
        idx = max(self._last(self.vm, t) for t in tags)
        if idx < self.vm_done:
            self.emit(VmWait(None))
            return
        n = len(self.vm) - 1 - idx
        assert n <= 63, n
        self.emit(VmWait(n))
        self.vm_done = idx + 1

    def need_lg(self, *tags):
        idx = max(self._last(self.lg, t) for t in tags)
        if idx < self.lg_done:
            return
        n = min(len(self.lg) - 1 - idx, 15)
        self.emit(f"s_waitcnt lgkmcnt({n})")
        self.lg_done = max(self.lg_done, len(self.lg) - n)

    def drain_lg(self):
        if self.lg_done < len(self.lg):
            self.emit("s_waitcnt lgkmcnt(0)")
            self.lg_done = len(self.lg)


def acc(m, n):
    b = (m * 16 + n) * 4
    if I8:
        return f"v[{VA_BASE + b}:{VA_BASE + b + 3}]"
    return f"a[{b}:{b + 3}]"


def acc_reg(m, n, i):
    """Register i (0..3: rows 4g+i of panel m) of the ArchVGPR accumulator of (panel m, query tile n) (int8 bodies)."""
    return f"v{VA_BASE + (m * 16 + n) * 4 + i}"


def ring(b, m):
    return f"%[x{b * MT + m}]"


# explicit scalar registers (listed as clobbers): descriptors need sub-register arithmetic
PRIO_STEPS = {8: (0, 2), 12: (1, 2), 16: (0, 1), 20: (1, 1), 24: (0, 0), 28: (1, 0)}   # fragment -> (wave half, priority)
XCUR, XNEXT, RNS, RET = "s[80:83]", "s[84:87]", "s[88:91]", "s[92:93]"
# zig-zag bodies: the direction of the tile whose k-steps the X cursors fetch / whose chunks are staged, in the two scratch
# SGPRs of the statement: XSTEP = what a chunk's second k-step adds to the cursors (0x400 upwards, -0xC00 downwards),
# QSTEP = +- one chunk of the query image
XSTEP, QSTEP = "%[sacc0]", "%[sacc1]"


def gen_pretest(s, n, part):
    """Admission pre-test of query tile n, folded into the tile's last k-step (int8 cosine and l2c).

    Exact test per row j and query: float(I_j) r_j + p_j >= T (the hit stub's arithmetic).  With r_j >= 0 and
    R = max_j r_j, P = max_j p_j over the lane's 8 rows (NaN = tombstoned rows drop out of v_max_f32),
    float(max(0, max_j I_j)) R + P >= float(I_j) r_j + p_j for every j (rounding is monotone), so a lane whose
    left-hand side stays below T holds no admissible row: 4 v_max3_i32 + cvt + fma + compare per query tile instead
    of 8 reads + 8 cvt + 8 fma + 5 max + compare, issued between the MFMAs of the following query tiles.  A lane
    that passes sends the wave to .Lhit<n>, which computes the 8 exact bounds and calls the append routine; on
    N(0,1) rows the pre-test lets ~2 % of the (wave, query tile) pairs through, the exact test 0.3 %.
    part 0 / 1: the halves issued after the first / second MFMA of the query tile two steps later."""
    a = s.emit
    regs = [acc_reg(m, n, i) for m in range(MT) for i in range(4)]
    if I8_SPACE == "ip":
        return gen_pretest_ip(s, n, part, regs)
    t0, t1 = (("%[e0]", "%[e1]") if n & 1 == 0 else ("%[e2]", "%[e3]"))
    if part == 0:
        a(f"v_max3_i32 {t0}, {regs[0]}, {regs[1]}, {regs[2]}")
        a(f"v_max3_i32 {t1}, {regs[3]}, {regs[4]}, {regs[5]}")
        a(f"v_max3_i32 {t0}, {t0}, {regs[6]}, {regs[7]}")
        if L2C:   # (A_j = I_j + e_j times ONE positive factor S SQ: no clamp at 0 needed, and none wanted)
            a(f"v_max_i32 {t0}, {t0}, {t1}")
        else:
            a(f"v_max3_i32 {t0}, {t0}, {t1}, 0")
    else:
        a(f"v_cvt_f32_i32 {t0}, {t0}")
        a(f"v_fma_f32 {t0}, {t0}, %[e10], %[e12]")
        a(f"v_cmp_ge_f32 vcc, {t0}, %[tq{n}]")
        a(f"s_cbranch_vccnz .Lhit{n}c{s.copy}_%=")
        a(f".Lback{n}c{s.copy}_%=:")


# ip folded pre-test: the e registers that only the serial admission test used (the append routine keeps e5..e9, e11)
# plus two of the tq pool (the thresholds come from LDS per query tile here; the statement declares IP_TQ of them)
IP_SMAX, IP_NMAX, IP_T0, IP_T1 = "%[e10]", "%[e12]", "%[e0]", "%[e1]"
IP_TQ = 4


def ip_consts(n):
    """(thr, ke) registers of query tile n's per-query constants: two sets, by parity."""
    return ("%[e2]", "%[e3]") if n & 1 == 0 else ("%[tq1]", "%[tq2]")


def ip_fetch(s, n):
    thr, ke = ip_consts(n)
    s.lds(f"ds_read_b32 {thr}, %[thra]" + (f" offset:{n * 64}" if n else ""), ("thr", n))
    s.lds(f"ds_read_b32 {ke}, %[thra] offset:{2048 + n * 64}", ("ke", n))


def gen_pretest_ip(s, n, part, regs):
    """Folded admission pre-test of query tile n, ip (int8).

    Exact test per row j (the hit stub, in this order of operations): u = float(I_j); u = u s_j; u = fma(ke, N_j, u);
    u >= thr, with s_j the row's scale, N_j = |x_j|, and ke, thr the lane's query's constants.  The pre-test runs the SAME
    operations on a virtual row that dominates the lane's 8 rows -- I* = max(0, max_j I_j), S = max_j s_j, N = max_j N_j:
    every operation is monotone in each of its inputs (ke >= 0; rounding is monotone), so its result is >= every row's u,
    and a lane whose virtual row stays below thr holds no admissible row.  It is as sharp as the rows of a lane group are
    alike: the shadow builder gives them one scale (shadow8_rows_kernel)."""
    a = s.emit
    thr, ke = ip_consts(n)
    if part == 0:
        a(f"v_max3_i32 {IP_T0}, {regs[0]}, {regs[1]}, {regs[2]}")
        a(f"v_max3_i32 {IP_T1}, {regs[3]}, {regs[4]}, {regs[5]}")
        a(f"v_max3_i32 {IP_T0}, {IP_T0}, {regs[6]}, {regs[7]}")
        a(f"v_max3_i32 {IP_T0}, {IP_T0}, {IP_T1}, 0")
        if n + 1 < NQT:
            ip_fetch(s, n + 1)
    else:
        a(f"v_cvt_f32_i32 {IP_T0}, {IP_T0}")
        a(f"v_mul_f32 {IP_T0}, {IP_T0}, {IP_SMAX}")
        s.need_lg(("ke", n), ("thr", n))
        a(f"v_fma_f32 {IP_T0}, {ke}, {IP_NMAX}, {IP_T0}")
        a(f"v_cmp_ge_f32 vcc, {IP_T0}, {thr}")
        a(f"s_cbranch_vccnz .Lhit{n}c{s.copy}_%=")
        a(f".Lback{n}c{s.copy}_%=:")


def max_tree(a, dst, src):
    """dst = the maximum of %[src0] .. %[src7] (NaN drops out)."""
    a(f"v_max3_f32 {dst}, %[{src}0], %[{src}1], %[{src}2]")
    a(f"v_max3_f32 {dst}, {dst}, %[{src}3], %[{src}4]")
    a(f"v_max3_f32 {dst}, {dst}, %[{src}5], %[{src}6]")
    a(f"v_max_f32 {dst}, {dst}, %[{src}7]")


def gen_rowmax_ip(s, part):
    """Start of the last k-step, ip: S = max s_j, N = max N_j over the lane's rows (NaN = tombstoned rows drop out of
    v_max_f32), and the constants of query tile 0."""
    if part == 1:
        max_tree(s.emit, IP_SMAX, "s")
        max_tree(s.emit, IP_NMAX, "r")
        ip_fetch(s, 0)


def gen_rowmax_l2c(s, part):
    """Start of the last k-step, l2c.  Loaded: u_j = the x-slots of the lane's 8 row pairs -- the group's scale S in the first
    panel's rows (u0..u3), the group's largest relative row error Bg in the second panel's (u4..u7), never NaN -- and r_j =
    |x_j| (NaN = dead row).  e10 = S SQ (the factor of the integer A = I + e); KEg = KEq + KEr Bg (the lane's error
    coefficient: the query part + the row part); r_j becomes c_j = KEg N_j + P0 with P0 = max_j -(1 - slack) N_j^2; e12 =
    max_j c_j.  Pre-test: float(max_j A_j) e10 + e12 >= thr; per row (stubs): float(A_j) e10 + c_j >= thr.  NaN rows drop out of
    every v_max; their c_j stays NaN and fails every compare."""
    a = s.emit
    NR = 4 * MT
    if part == 0:
        a("v_mul_f32 %[e10], %[sqc], %[u0]")                 # S SQ
        a("v_mov_b32 %[e4], %[kec]")                         # (one SGPR per VALU instruction: the constant-bus limit)
        a("v_fma_f32 %[e4], %[krc], %[u4], %[e4]")           # KEg = KEr Bg + KEq
        for j in range(NR):
            a(f"v_mul_f32 %[u{j}], %[r{j}], %[r{j}]")
        for j in range(NR):
            a(f"v_mul_f32 %[u{j}], 0xbf7fffe0, %[u{j}]")    # -(1 - 2^-19) = -(1.0f - kSlack): the constant of scan_epilogue and of filter_l2_offsets_kernel
    else:
        max_tree(a, "%[e12]", "u")                          # P0
        for j in range(NR):
            a(f"v_fma_f32 %[r{j}], %[e4], %[r{j}], %[e12]")
        max_tree(a, "%[e12]", "r")


def gen_rowmax(s, part):
    """Start of the last k-step: p_j *= K, then R = max r_j and P = max p_j over this lane's rows (e10, e12)."""
    if L2C:
        return gen_rowmax_l2c(s, part)
    if I8_SPACE == "ip":
        return gen_rowmax_ip(s, part)
    a = s.emit
    if part == 0:
        for j in range(4 * MT):
            a(f"v_mul_f32 %[p{j}], %[k1], %[p{j}]")
    else:
        max_tree(a, "%[e10]", "r")
        max_tree(a, "%[e12]", "p")


def q_schedule(nkc, bufs):
    """Which Q chunk a tile computes at each chunk position, where it sits in LDS and what is staged meanwhile.

    nkc: 128-column chunks of the image (ld8 / 128, even); bufs: chunk buffers in LDS.  Returns table[parity][p] =
    (chunk, buffer, stage) for the workgroup's even (parity 0) / odd (1) tiles; stage = (chunk, buffer) sent L2 -> LDS during
    position p, or None.  Integer accumulation is exact and associative, so the order of the chunks is free: even tiles
    ascend, odd tiles descend, and the `bufs` chunks a tile ends on are the ones the next tile starts on.  Chunk c always
    sits in buffer c % bufs (any `bufs` consecutive chunks are distinct there); a chunk is staged one position before its
    use unless it is still resident from the turn.  The prologue stages chunks 0 .. min(nkc, bufs) - 1; with nkc <= bufs
    nothing is ever staged again.  The buffer written at position p held the chunk used at position p - bufs + 1: never
    the current one, and its last read lies behind at least one chunk barrier."""
    assert nkc >= 2 and nkc % 2 == 0 and bufs in (2, 3, 4)
    table = []
    for parity in (0, 1):
        rows = []
        for p in range(nkc):
            c = p if parity == 0 else nkc - 1 - p
            nxt = c + 1 if parity == 0 else c - 1                      # the chunk of position p + 1
            turn = range(bufs) if parity == 0 else range(nkc - bufs, nkc)   # resident when the tile starts
            stage = (nxt, nxt % bufs) if 0 <= nxt < nkc and nxt not in turn else None
            rows.append((c, c % bufs, stage))
        table.append(rows)
    return table


def body_stage_flags(bufs=None):
    """The bodies are generic over nkc (a tile = first body, nkc/2 - 2 middle bodies, last body; or the single body of nkc = 2),
    two chunk positions each: whether a position stages must therefore depend on the body alone -- not on nkc, not on the
    tile's direction.  Read from q_schedule, and checked for every nkc."""
    bufs = bufs or Q_BUFS
    flags = {}
    # (four buffers: the positions that stage depend on nkc -- the bodies exist for Q4_NKC alone, first / mid / last once each)
    for nkc in ((Q4_NKC,) if bufs == 4 else (2, 4, 6, 8, 10, 16, 32)):
        for rows in q_schedule(nkc, bufs):
            st = [r[2] is not None for r in rows]
            kinds = {"single": st} if nkc == 2 else {"first": st[:2], "last": st[-2:],
                                                     **{f"mid{i}": st[i:i + 2] for i in range(2, nkc - 2, 2)}}
            for kind, f in kinds.items():
                kind = kind.rstrip("0123456789")
                assert flags.setdefault(kind, tuple(f)) == tuple(f), (nkc, kind, f, flags)
    return flags


def q4_barrier_flags(sparse=None):
    """Four-buffer bodies: after which chunk positions of a tile the workgroup meets at an s_barrier, per body.  Two rules:
      1. a transfer into a buffer is issued only after a barrier that every wave reaches after its last read of the chunk
         that buffer held;
      2. a staged chunk is first read only after a barrier that every wave reaches after its own vmcnt wait for its pieces.
    The transfer of position p goes into the buffer that position p - 3 read (four buffers, one chunk ahead), and is first
    read at p + 1: rule 2 asks for a barrier after every position that stages (the wait sits right before it), rule 1 for one
    between positions p - 3 and p -- the one after position 1 serves both transfers (positions 3 and 4).  Not sparse: one
    barrier after every position, as in the two-buffer bodies."""
    sparse = Q4_SPARSE_BARRIERS if sparse is None else sparse
    stage = [r[2] is not None for r in q_schedule(Q4_NKC, 4)[0]]
    assert stage == [r[2] is not None for r in q_schedule(Q4_NKC, 4)[1]] == [False, False, False, True, True, False]
    bar = [(not sparse) or stage[p] or p == 1 for p in range(Q4_NKC)]
    return {"first": tuple(bar[0:2]), "mid": tuple(bar[2:4]), "last": tuple(bar[4:6])}


def dma_pieces():
    """This wave's LDS-DMA transfers per chunk: (set name, index, byte offset inside the chunk / the LDS buffer).
    A chunk is 2 * NQT fragments of 1 KiB at n * 2048 + h * 1024 (the image keeps the 16-tile layout whatever NQT is).
    NQT = 16: wave w moves tiles w and w + NW, both halves (4 transfers); NQT = 8: tile w, both halves (2); NQT = 4: ONE
    fragment -- tile w & 3, half w >> 2: the wrapper puts that into the wave's base offsets (qvoff / wave2k), offset 0 here.
    Every wave issues the same number of transfers: the counted vmcnt waits assume identical issue sequences."""
    if NQT == 16:
        return [(sn, i, i * NW * 2048 + half * 1024) for sn, half in (("qb", 0), ("qa", 1)) for i in range(2)]
    if NQT == 8:
        return [("qb", 0, 0), ("qa", 0, 1024)]
    return [("qb", 0, 0)]


def gen_chunk(s, R, step0, zero_first, last, final, turn=False, stage=True, barrier=True):
    """One 64-column chunk = 2 k-steps = 2 * NQT fragments x MT MFMAs.  final: the tile's last chunk, whose second k-step
    carries the admission pre-tests (int8).  Zig-zag bodies: turn = the tile's first chunk, which sits in the buffer the
    previous tile ended on (no toggle); stage = whether this position sends a chunk to the other buffer (q_schedule)."""
    assert ZZ or (stage and not turn)
    assert barrier or QB == 4
    if not turn and QB == 4:
        # Chunk c sits in buffer c & 3: the read base moves one buffer in the tile's direction (QSTEP = +- 0x8000, uniform over
        # the workgroup) and wraps at 128 KiB; lane16 < 0x8000 rides along.  Transfers only ever go to buffers 0 and 1, and
        # alternately: the toggle at every position but a tile's first leaves sldw on buffer 0 at an upward tile's position 3
        # (chunk 4) and on buffer 1 at a downward tile's (chunk 1) -- five toggles per tile, and the prologue starts it on buffer 1.
        s.emit(f"v_add_u32 %[ldr], {QSTEP}, %[ldr]")
        s.emit("v_and_b32 %[ldr], 0x1ffff, %[ldr]")
        s.emit("s_xor_b32 %[sldw], %[sldw], 0x8000")
    elif not turn:
        s.emit("v_xor_b32 %[ldr], 0x8000, %[ldr]")
        s.emit("s_xor_b32 %[sldw], %[sldw], 0x8000")

    NF = 2 * NQT   # fragments per chunk: NQT query tiles x 2 k-steps (k-step major)

    def read(f):
        h, n = f // NQT, f % NQT
        s.lds(f"ds_read_b128 %[t{f % QD}], %[ldr] offset:{n * 2048 + h * 1024}", ("rd", f))

    def refill(h):
        step = step0 + h
        b = step % R
        if ZZ:
            # One cursor per panel for the whole stream: k-step R ahead of the one just computed, in EXECUTED order.  A
            # tile walks its chunks up or down but the two k-steps inside a chunk always upwards (the fragment offsets in
            # LDS stay what they are): + 0x400 after a chunk's first k-step, XSTEP (+ 0x400 / - 0xC00) after its second.
            # In the tile's last body the cursor already walks the workgroup's next tile (gen_body), through XNEXT.
            for m in range(MT):
                s.vmem(f"buffer_load_dwordx4 {ring(b, m)}, %[lane16], {XNEXT if last else XCUR}, %[xso{m}] offen nt", ("x", b, m))
            for m in range(MT):
                s.emit(f"s_add_u32 %[xso{m}], %[xso{m}], " + ("0x400" if h == 0 else XSTEP))
            return
        for m in range(MT):
            if last:   # the workgroup's next tile: k-step `step` (< R <= 4: fits the instruction offset)
                so = "0" if m == 0 else "%[pb]"
                off = f" offset:{step * 1024}" if step else ""
                s.vmem(f"buffer_load_dwordx4 {ring(b, m)}, %[lane16], {XNEXT}, {so} offen{off} nt", ("x", b, m))
            else:
                s.vmem(f"buffer_load_dwordx4 {ring(b, m)}, %[lane16], {XCUR}, %[xso{m}] offen nt", ("x", b, m))
        if not last:
            for m in range(MT):
                s.emit(f"s_add_u32 %[xso{m}], %[xso{m}], 0x400")

    # LDS-DMA staging: chunk c+1 goes global -> LDS directly (buffer_load ... lds: LDS address = M0 + 16*lane), early in
    # chunk c; no staging registers, no ds_write (tools/probe: +5 % on the bare loop).  Fragment index -> transfer.
    plan = {2 + i: piece for i, piece in enumerate(dma_pieces())}

    prio = I8
    if prio:
        s.emit("s_setprio 3")
    for f0 in range(QD):
        read(f0)
    prio_steps = {k * NF // 32: v for k, v in PRIO_STEPS.items()}
    for f in range(NF):
        h, n = f // NQT, f % NQT
        b = (step0 + h) % R
        if prio and f in prio_steps:
            # The two waves of a SIMD share its MFMA pipe and issue is arbitrated by priority, then age: priority that
            # falls with progress (3, 2, 1, 0 per quarter chunk), the younger wave's steps half a quarter later, makes the
            # two leapfrog every 4 fragments.  (On the bf16 body it made the scan 3 % SLOWER: the kernel is power-bound,
            # tools/probe, cycles saved come back as a lower clock.)
            who, level = prio_steps[f]
            s.emit(f"s_cmp_eq_u32 %[wtype], {who}")
            s.emit(f"s_cbranch_scc0 .Lp{s.label}_%=")
            s.emit(f"s_setprio {level}")
            s.emit(f".Lp{s.label}_%=:")
            s.label += 1
        if n == 0:
            s.need_vm(*[("x", b, m) for m in range(MT)])
            if final and h == 1:   # issued before this body's ring refills: landed with them (vmcnt completes in order)
                s.need_vm(*[("rn", j) for j in range(4 * MT)])
        s.need_lg(("rd", f))
        for m in range(MT):
            c = ("%[eo" + str(m) + "]" if L2C else "0") if (zero_first and h == 0) else acc(m, n)
            op = "v_mfma_i32_16x16x64_i8" if I8 else "v_mfma_f32_16x16x32_bf16"
            s.emit(f"{op} {acc(m, n)}, {ring(b, m)}, %[t{f % QD}], {c}")
            if final and h == 1:
                # the accumulators of query tile n - 2 are complete (their last MFMAs were issued four MFMAs ago)
                if n < 2:
                    if m == 1:
                        gen_rowmax(s, n)
                else:
                    gen_pretest(s, n - 2, m)
        if f + QD < NF:
            read(f + QD)
        if f in plan and stage:
            setname, i, const = plan[f]
            s.emit(f"s_add_u32 m0, %[sldw], 0x{const:x}")
            s.emit(f"s_add_u32 %[st0], %[qcur], 0x{const:x}")
            s.vmem("buffer_load_dwordx4 %[qvoff], %[qsrd], %[st0] offen lds", (setname, i))
        if n == NQT - 1:
            refill(h)
    if final:   # the last two query tiles: nothing left to hide behind
        gen_pretest(s, NQT - 2, 0)
        gen_pretest(s, NQT - 2, 1)
        s.emit("s_nop 7")   # XDL write (the last query tile's MFMAs, 8 instructions back) -> VALU read: 16 wait states with this
        #                     (an 8-pass MFMA needs 11; once per tile, so the margin is free)
        gen_pretest(s, NQT - 1, 0)
        gen_pretest(s, NQT - 1, 1)
    # advance the Q cursor (chunk c+2 -> c+3, wrapping) and publish the chunk just staged
    if ZZ:
        if stage:   # (a position that stages nothing issues no transfer and waits for none)
            s.emit(f"s_add_u32 %[qcur], %[qcur], {QSTEP}")   # the next chunk in the tile's direction: no wrap inside a tile
            s.need_vm(*[(sn, i) for sn, i, _ in dma_pieces()])
    else:
        s.emit("s_add_u32 %[qcur], %[qcur], 0x8000")
        s.emit("s_cmp_eq_u32 %[qcur], %[qbytes]")
        s.emit("s_cselect_b32 %[qcur], 0, %[qcur]")
        s.need_vm(*[(sn, i) for sn, i, _ in dma_pieces()])   # this wave's share of the chunk staged since the last barrier
    s.drain_lg()
    if barrier:
        s.emit("s_barrier")


def gen_eo_loads(s):
    """l2c: the per-row integer offsets of this wave's 32 rows of the NEXT tile (the last tile of a workgroup re-reads its own:
    harmless) -> the two 4-register tuples eo0 / eo1, which are the C operands of that tile's first k-step.  They live in the
    same allocation as the row pairs, 8 x capacity bytes further on; the SGPR `eo` holds that distance less 4 x (the wave's
    first row), so that one descriptor (the row pairs') serves both."""
    s.emit("v_lshrrev_b32 %[e0], 1, %[rnvoff]")       # 16 g: this lane's 4 rows x 4 bytes inside a panel's 64
    s.emit("s_lshr_b32 %[st0], %[rnstride], 1")        # the next tile's rows: 4 bytes per row where the pairs have 8
    s.emit("s_cmp_gt_u32 %[tl], 1")
    s.emit("s_cselect_b32 %[st0], %[st0], 0")
    s.emit("s_add_u32 %[st0], %[st0], %[eo]")
    for m in range(MT):
        s.vmem(f"buffer_load_dwordx4 %[eo{m}], %[e0], {RNS}, %[st0] offen" + (f" offset:{64 * m}" if m else ""), ("eo", m))


def gen_body(s, R, first, last):
    if ZZ and last:
        # From here on the X cursors fetch the workgroup's NEXT tile, which walks the other way: its first executed k-step
        # is column step 0 (upwards) or the first of its last chunk, 2 nkc - 2 = qbytes / 0x4000 - 2 (downwards) -- all of it
        # in the scalar offset, so one instruction serves both directions.
        s.emit(f"s_sub_u32 {XSTEP}, 0xfffff800, {XSTEP}")     # 0x400 <-> -0xC00
        s.emit("s_lshr_b32 %[st0], %[qbytes], 4")
        s.emit("s_sub_u32 %[st0], %[st0], 0x800")
        s.emit(f"s_cmp_eq_u32 {XSTEP}, 0x400")
        s.emit("s_cselect_b32 %[xso0], 0, %[st0]")
        s.emit("s_add_u32 %[xso1], %[pb], %[xso0]")
    if last and L2C and not first:
        # issued before the row-pair loads below: in-order completion makes the wait for those a wait for these too.  (The
        # offsets in the registers now were last read in this tile's FIRST k-step, which is not in this body.)
        gen_eo_loads(s)
    if last:
        # |x| of this lane's 4*MT rows (rows 4g..4g+3 of every panel) for the admission test
        for j in range(4 * MT):
            off = (j >> 2) * 64 + (j & 3) * 4
            if I8:
                # per-row pairs {a, b}: cosine {sx/(|x|+1e-30), the row's own error}; ip {sx, |x|}; l2c {the group's
                # scale / error (gen_rowmax_l2c), |x|} (NaN: tombstoned)
                a_reg = {"cosine": f"r{j}", "ip": f"s{j}", "l2": f"u{j}"}[I8_SPACE]
                b_reg = f"p{j}" if I8_SPACE == "cosine" else f"r{j}"
                s.vmem(f"buffer_load_dword %[{a_reg}], %[rnvoff], {RNS}, 0 offen" + (f" offset:{2 * off}" if off else ""), ("rn", j))
                s.vmem(f"buffer_load_dword %[{b_reg}], %[rnvoff], {RNS}, 0 offen offset:{2 * off + 4}", ("rn", j))
                continue
            s.vmem(f"buffer_load_dword %[r{j}], %[rnvoff], {RNS}, 0 offen" + (f" offset:{off}" if off else ""),
                   ("rn", j))
    for ch in range(R // 2):
        if last and L2C and first and ch == 1:   # a one-body tile: its own offsets were read in chunk 0's first k-step
            gen_eo_loads(s)
        if ZZ:
            kind = ("single" if last else "first") if first else ("last" if last else "mid")
            gen_chunk(s, R, 2 * ch, first and ch == 0, last, last and ch == R // 2 - 1, turn=first and ch == 0,
                      stage=body_stage_flags(QB)[kind][ch], barrier=QB != 4 or q4_barrier_flags()[kind][ch])
            continue
        gen_chunk(s, R, 2 * ch, first and ch == 0, last, I8 and last and ch == R // 2 - 1)
    if last:
        s.need_vm(*([("rn", j) for j in range(4 * MT)] + ([("eo", m) for m in range(MT)] if L2C else [])))


FIRST, MID, LAST, SINGLE = (True, False), (False, False), (False, True), (True, True)   # (first, last) of a tile's bodies


def histories(first, last):
    """The body sequences that can run before a body, two deep (every target of a counted wait -- ring slot, Q set, row
    pairs -- was issued at most one body earlier).  bf16 bodies: every body issues the middle body's pattern of ring and Q
    operations.  Zig-zag bodies do not (a position that stages nothing issues fewer), so every real predecessor sequence is
    simulated.  A workgroup's first tile follows the prologue's vmcnt(0): its queue holds less than any history here, which
    only makes a counted wait stricter than needed."""
    if not ZZ:
        return [[MID, MID]]
    if QB == 4:   # a tile is first, mid, last, once each (Q4_NKC chunks): one predecessor sequence per body
        return [{FIRST: [MID, LAST], MID: [LAST, FIRST], LAST: [FIRST, MID]}[(first, last)]]
    if (first, last) == SINGLE:
        return [[SINGLE, SINGLE]]
    if first:
        return [[FIRST, LAST], [MID, LAST]]
    return [[LAST, FIRST], [FIRST, MID], [MID, MID]]


def body_lines(R, first, last, label0=0):
    variants = []
    for hist in histories(first, last):
        s = Sched()
        s.recording = False
        for f, l in hist:
            gen_body(s, R, f, l)
        s.recording = True
        s.label = label0
        s.copy = str(label0)
        gen_body(s, R, first, last)
        variants.append(s.lines)
    return merge_waits(variants)


def gen_admission(space):
    """bf16 bodies, after the k-loop of a tile: bounds, quick reject per query tile, calls into .Lslow.  (The int8 bodies
    run their pre-tests inside the last k-step: gen_pretest.)"""
    s = Sched()
    a = s.emit
    a("s_nop 15")   # XDL write -> v_accvgpr_read of the accumulators
    a("s_nop 7")
    # ke = the query's error term from LDS (prep_query_state).  Per-row constants (scan_epilogue):
    # cosine p0 = 1/(|x|+1e-30), u = a*p0 + ke; ip p0 = |x|, u = a + ke*p0; l2 p0 = |x|, p1 = -|x|^2 (1-slack),
    # u = sq*(a + ke*p0) + p1
    NR = 4 * MT
    for j in range(NR):
        if space == "cosine":
            a(f"v_add_f32 %[r{j}], 0x0da24260, %[r{j}]")   # + 1e-30f
            a(f"v_rcp_f32 %[r{j}], %[r{j}]")
        elif space == "l2":
            a(f"v_mul_f32 %[p{j}], %[r{j}], %[r{j}]")
            a(f"v_mul_f32 %[p{j}], %[k1], %[p{j}]")        # k1 = -(1 - slack)
    thr = lambda n: f"%[e{n & 1}]"
    sq = lambda n: f"%[e{2 + (n & 1)}]"
    ke = lambda n: f"%[e{10 if n & 1 else 12}]"

    def fetch(n):
        s.lds(f"ds_read_b32 {thr(n)}, %[thra] offset:{n * 64}", ("thr", n))
        s.lds(f"ds_read_b32 {ke(n)}, %[thra] offset:{2048 + n * 64}", ("ke", n))
        if space == "l2":
            s.lds(f"ds_read_b32 {sq(n)}, %[thra] offset:{1024 + n * 64}", ("sq", n))

    fetch(0)
    for n in range(NQT):
        if n + 1 < NQT:
            fetch(n + 1)
        for j in range(NR):
            m, i = j >> 2, j & 3
            a(f"v_accvgpr_read_b32 %[u{j}], a{(m * 16 + n) * 4 + i}")
        s.need_lg(("ke", n), *([("sq", n)] if space == "l2" else []))
        for j in range(NR):
            if space == "cosine":
                a(f"v_fma_f32 %[u{j}], %[u{j}], %[r{j}], {ke(n)}")
            elif space == "ip":
                a(f"v_fma_f32 %[u{j}], {ke(n)}, %[r{j}], %[u{j}]")
            else:
                a(f"v_fma_f32 %[u{j}], {ke(n)}, %[r{j}], %[u{j}]")
                a(f"v_fma_f32 %[u{j}], {sq(n)}, %[u{j}], %[p{j}]")
        a("v_max3_f32 %[e4], %[u0], %[u1], %[u2]")
        a("v_max3_f32 %[e5], %[u3], %[u4], %[u5]")
        for j in range(6, NR, 4):   # two dependency chains
            a(f"v_max3_f32 %[e4], %[u{j}], %[u{j + 1}], %[e4]")
            if j + 3 < NR:
                a(f"v_max3_f32 %[e5], %[u{j + 2}], %[u{j + 3}], %[e5]")
        a("v_max_f32 %[e4], %[e4], %[e5]")
        s.need_lg(("thr", n))
        a(f"v_cmp_ge_f32 vcc, %[e4], {thr(n)}")
        a(f"s_cbranch_vccnz .Lhit{n}_%=")
        a(f".Lback{n}_%=:")
    return s.lines


def gen_hit_stubs(copy=""):
    out = []
    for n in range(NQT):
        out.append(f".Lhit{n}{copy}_%=:")
        if I8 and I8_SPACE != "ip":   # the pre-test let a lane through: the 8 exact bounds of this query tile (cosine, l2c)
            for j in range(4 * MT):
                out.append(f"v_cvt_f32_i32 %[u{j}], {acc_reg(j >> 2, n, j & 3)}")
            for j in range(4 * MT):   # (l2c: float(A_j) S SQ + c_j, the pre-test's own arithmetic per row: gen_rowmax_l2c)
                out.append(f"v_fma_f32 %[u{j}], %[u{j}], " + ("%[e10], %[r" + str(j) + "]" if L2C else f"%[r{j}], %[p{j}]"))
            # Most calls are false alarms of the pre-test (it tests a row that dominates the lane's 8): one max tree
            # and one compare send those straight back, instead of through the append routine's 8 compares and 8
            # skipped row blocks (a taken branch each).  All 8 waves meet at the next barrier, so a tile is as slow
            # as the wave with the most stub calls: the call's length is what counts.
            out += ["v_max3_f32 %[e4], %[u0], %[u1], %[u2]", "v_max3_f32 %[e5], %[u3], %[u4], %[u5]",
                    "v_max3_f32 %[e4], %[u6], %[u7], %[e4]", "v_max_f32 %[e4], %[e4], %[e5]",
                    f"v_cmp_ge_f32 vcc, %[e4], %[tq{n}]", f"s_cbranch_vccz .Lback{n}{copy}_%="]
        elif I8:   # ip: the same, with the constants the pre-test holds in registers (gen_pretest_ip)
            thr, ke = ip_consts(n)
            for j in range(4 * MT):
                out.append(f"v_cvt_f32_i32 %[u{j}], {acc_reg(j >> 2, n, j & 3)}")
            for j in range(4 * MT):
                out.append(f"v_mul_f32 %[u{j}], %[u{j}], %[s{j}]")
            for j in range(4 * MT):
                out.append(f"v_fma_f32 %[u{j}], {ke}, %[r{j}], %[u{j}]")
        thr_src = (f"%[tq{n}]" if I8_SPACE != "ip" else ip_consts(n)[0]) if I8 else f"%[e{n & 1}]"
        out += [f"v_mov_b32 %[e6], {thr_src}",          # the threshold of this query tile
                f"s_movk_i32 %[sn64], 0x{n * 16:x}",      # first query of this tile
                f"s_getpc_b64 {RET}",
                "s_add_u32 s92, s92, 12",                 # return to the instruction after the branch below
                "s_addc_u32 s93, s93, 0",
                "s_branch .Lslow_%=",
                f"s_branch .Lback{n}{copy}_%="]
    return out


def lds_stage_cap(bufs=None):
    """Entries of a wave's staging area in LDS (12 B each, SoA): what is left of the 160 KiB per CU beside `bufs` Q buffers
    (default: the body being generated)."""
    bufs = bufs or QB
    wgs_per_cu = (16 // MT) // NW      # two waves per SIMD
    per_wg = (160 * 1024) // wgs_per_cu - (bufs * CHUNK_BYTES + 3072)   # Q buffers + thr[256], qscale[256], ke[256]
    return min(WG_CAP // NW, (per_wg // NW) // 12 // 8 * 8)


def gen_slow():
    """u0.. = bounds of this lane's 4*MT rows for query sn64 + c16, e6 = threshold.

    Wave-private append: the wave keeps its entry count in an SGPR; per row j the passing lanes form
    an SGPR mask and take the slots count + (passing lanes below), via v_mbcnt -- no atomics.
    The first LCW entries of a launch are staged in LDS (u[], row[], q[]) and copied to the wave's
    global buffer when the kernel ends: a global store inside the loop would sit in the vmcnt queue
    behind the prefetched loads for ~1-2 us and turn every counted wait into a drain of the X
    prefetch (measured: 17 % of the scan).  Entries beyond the staging area go straight to global
    memory (same slot numbering), entries beyond the global buffer flag their query as overflowed."""
    capw = WG_CAP // NW
    lcw = lds_stage_cap()
    o = [".Lslow_%=:",
         "v_add_u32 %[e9], %[sn64], %[c16v]",                       # e9 = query
         "v_add_u32 %[e11], %[trow], %[crow]"]                      # e11 = this lane's first row
    for j in range(4 * MT):                                         # one mask register pair per row
        o.append(f"v_cmp_ge_f32_e64 s[{60 + 2 * j}:{61 + 2 * j}], %[u{j}], %[e6]")
    for j in range(4 * MT):
        lo, hi = 60 + 2 * j, 61 + 2 * j
        o += [f"s_bcnt1_i32_b64 %[st0], s[{lo}:{hi}]",
              f"s_cbranch_scc0 .Lskip{j}_%=",
              f"s_mov_b64 exec, s[{lo}:{hi}]",
              f"v_mbcnt_lo_u32_b32 %[e8], s{lo}, 0",
              f"v_mbcnt_hi_u32_b32 %[e8], s{hi}, %[e8]",
              "v_add_u32 %[e8], %[wcnt], %[e8]",                    # e8 = this entry's slot
              f"v_add_u32 %[e5], {16 * (j >> 2) + (j & 3)}, %[e11]",  # e5 = row
              f"v_cmp_gt_u32 vcc, 0x{lcw:x}, %[e8]",
              "s_and_b64 exec, exec, vcc",                          # slots inside the LDS staging area
              "v_lshl_add_u32 %[e7], %[e8], 2, %[stg]",
              f"ds_write_b32 %[e7], %[u{j}]",
              f"ds_write_b32 %[e7], %[e5] offset:{lcw * 4}",
              f"ds_write_b32 %[e7], %[e9] offset:{lcw * 8}",
              f"s_andn2_b64 exec, s[{lo}:{hi}], vcc",               # the rest
              f"s_cbranch_execz .Lnext{j}_%=",
              f"v_cmp_gt_u32 vcc, 0x{capw:x}, %[e8]",
              f"s_mov_b64 s[76:77], exec",
              "s_and_b64 exec, exec, vcc",                          # slots inside the global buffer
              "v_lshlrev_b32 %[e7], 2, %[e8]",
              f"global_store_dword %[e7], %[u{j}], %[wgbu]",
              "global_store_dword %[e7], %[e5], %[wgbr]",
              "global_store_dword %[e7], %[e9], %[wgbq]",
              "s_andn2_b64 exec, s[76:77], vcc",                    # slots past the buffer
              "v_lshlrev_b32 %[e7], 2, %[e9]",
              "v_mov_b32 %[e5], 1",
              "global_store_dword %[e7], %[e5], %[ovfb]",           # overflow[q] = 1: the query is re-run exactly
              "s_mov_b64 exec, -1",
              "s_waitcnt vmcnt(0)",   # stores may complete before older loads: no counted vmcnt wait may see them
              f".Lnext{j}_%=:",
              "s_add_u32 %[wcnt], %[wcnt], %[st0]",
              f".Lskip{j}_%=:",
              "s_mov_b64 exec, -1"]
    o += ["s_mov_b64 exec, -1", f"s_setpc_b64 {RET}"]
    return o


def gen_slow_fast():
    """gen_slow with the common case as a straight line (int8 bodies).  A call appends, typically, ONE entry: one row of one lane.
    gen_slow walks 8 row blocks and skips the 7 empty ones with a taken branch each, and inside the one block that has a hit
    it takes another (no entry beyond the LDS staging area); all 8 waves of the workgroup meet at the next chunk barrier, so
    a tile is as slow as the wave with the most calls (phase stamps, profiles/r03: 11.2 us per tile in the second scan round,
    8 calls per wave and tile, against 9.3 us in the third with 1.3).  Here an empty row costs two scalar instructions and a
    branch that is NOT taken; the row blocks sit out of line, their own rare part (slots beyond the staging area) too."""
    capw = WG_CAP // NW
    lcw = lds_stage_cap()
    NR = 4 * MT
    o = [".Lslow_%=:",
         "v_add_u32 %[e9], %[sn64], %[c16v]",                       # e9 = query
         "v_add_u32 %[e11], %[trow], %[crow]"]                      # e11 = this lane's first row
    for j in range(NR):
        o.append(f"v_cmp_ge_f32_e64 s[{60 + 2 * j}:{61 + 2 * j}], %[u{j}], %[e6]")
    for j in range(NR):
        lo, hi = 60 + 2 * j, 61 + 2 * j
        o += [f"s_cmp_lg_u64 s[{lo}:{hi}], 0",
              f"s_cbranch_scc1 .Lrow{j}_%=",
              f".Lrowret{j}_%=:"]
    o.append(f"s_setpc_b64 {RET}")
    for j in range(NR):
        lo, hi = 60 + 2 * j, 61 + 2 * j
        o += [f".Lrow{j}_%=:",
              f"s_bcnt1_i32_b64 %[st0], s[{lo}:{hi}]",
              f"s_mov_b64 exec, s[{lo}:{hi}]",
              f"v_mbcnt_lo_u32_b32 %[e8], s{lo}, 0",
              f"v_mbcnt_hi_u32_b32 %[e8], s{hi}, %[e8]",
              "v_add_u32 %[e8], %[wcnt], %[e8]",                    # e8 = this entry's slot
              f"v_add_u32 %[e5], {16 * (j >> 2) + (j & 3)}, %[e11]",  # e5 = row
              f"v_cmp_gt_u32 vcc, 0x{lcw:x}, %[e8]",
              "s_and_b64 exec, exec, vcc",                          # slots inside the LDS staging area
              "v_lshl_add_u32 %[e7], %[e8], 2, %[stg]",
              f"ds_write_b32 %[e7], %[u{j}]",
              f"ds_write_b32 %[e7], %[e5] offset:{lcw * 4}",
              f"ds_write_b32 %[e7], %[e9] offset:{lcw * 8}",
              f"s_andn2_b64 exec, s[{lo}:{hi}], vcc",               # the rest: none, unless the staging area is full
              f"s_cbranch_execnz .Lovf{j}_%=",
              f".Lovfret{j}_%=:",
              "s_add_u32 %[wcnt], %[wcnt], %[st0]",
              "s_mov_b64 exec, -1",
              f"s_branch .Lrowret{j}_%="]
    for j in range(NR):
        o += [f".Lovf{j}_%=:",
              f"v_cmp_gt_u32 vcc, 0x{capw:x}, %[e8]",
              "s_mov_b64 s[76:77], exec",
              "s_and_b64 exec, exec, vcc",                          # slots inside the global buffer
              "v_lshlrev_b32 %[e7], 2, %[e8]",
              f"global_store_dword %[e7], %[u{j}], %[wgbu]",
              "global_store_dword %[e7], %[e5], %[wgbr]",
              "global_store_dword %[e7], %[e9], %[wgbq]",
              "s_andn2_b64 exec, s[76:77], vcc",                    # slots past the buffer
              "v_lshlrev_b32 %[e7], 2, %[e9]",
              "v_mov_b32 %[e5], 1",
              "global_store_dword %[e7], %[e5], %[ovfb]",           # overflow[q] = 1: the query is re-run exactly
              "s_mov_b64 exec, -1",
              "s_waitcnt vmcnt(0)",   # stores may complete before older loads: no counted vmcnt wait may see them
              f"s_branch .Lovfret{j}_%="]
    return o


def generate(space, R, i8=False, nqt=16, l2c=False, qbufs=2):
    """One body: bf16 (i8 False; R = 4, or 2 for an odd number of chunks) or int8 (R = 4; nqt query tiles; l2: l2c).

    i8: the 64*MT accumulator registers are ArchVGPRs, named explicitly (v[VA_BASE:...], clobbered), and the MFMA operands --
    the X ring and the B fragments, which only loads and MFMAs ever touch -- are AccVGPRs (loads may target them: MUBUF / DS
    acc bit).  An MFMA's C and D must be of one register class (the assembler rejects v-dst with a-srcC), so "results
    straight into VGPRs" means the whole accumulator lives there; the admission test then reads it with no v_accvgpr_read
    and no XDL drain, and is folded into the tile's last k-step (gen_pretest).  With two waves per SIMD the kernel descriptor
    becomes 192 ArchVGPRs + 48 AccVGPRs (accum_offset 192) instead of hipcc's 128 / 128 split.  The int8 bodies also run
    progress-based wave priorities (gen_chunk), hit stubs that leave at once when none of the 8 exact bounds passes
    (gen_hit_stubs) and the straight-line append routine (gen_slow_fast).

    nqt (int8): passes of <= 64 / <= 128 queries compute 4 / 8 of the 16 query tiles.  The empty tiles' MFMAs, B reads, Q
    transfers and admission tests are simply not generated; chunks, barriers, the ring and the image layout stay (a chunk
    period is then ~3,300 cycles of HBM stream against ~250 of MFMAs: the body is a pure stream of the shadow).

    l2c (int8 l2): the exact test of row j is  sq (I_j S + ke N_j) + p_j >= thr,  p_j = -(1 - slack) N_j^2; a dominating-row
    pre-test with P0 = max_j p_j would be loose by the spread of the norms inside a lane (one sigma of the score).  With
    e_j = ceil((p_j - P0) / (SQ S)) + 1 (SQ = the pass's largest sq; <= 0; filter_l2_offsets_kernel, once per pass) added to
    the integer dot product -- the first k-step's MFMAs take the lane's e_j as their C operand instead of 0 --
      u'_j = sq ((I_j + e_j) S + ke N_j) + P0  >=  sq (I_j S + ke N_j) + p_j      for every query of the pass (sq <= SQ),
    an upper bound of the row's score that differs from the exact test's by ~two quanta sq S; it is what the pre-test
    dominates (one scale S per lane: the shadow builder groups l2 rows like ip's) and what the stubs append.  The prep
    quantises every query of the pass with one step, so that sq = SQ for all of them, and one error coefficient
    KE = max_q 2 |q| ke_q stands for every query's: u'_j = float(I_j + e_j) (S SQ) + (KE N_j + P0).  The per-query constants
    shrink to the threshold, kept in registers for the launch like cosine's; S SQ and KE N_j + P0 are formed once per row
    tile (gen_rowmax_l2c).  SQ, KE: scalars of the pass (filter_l2_offsets_kernel).

    qbufs = 4 (int8, nqt = 16; an image of exactly Q4_NKC = 6 chunks, ld8 = 768): four chunk buffers at 0 / 32 / 64 / 96 KiB,
    chunk c in buffer c & 3.  The prologue stages chunks 0..3; chunks 2 and 3 are never written again, a tile stages two
    chunks (4 and 5 on the way up, 1 and 0 on the way down, into buffers 0 and 1) instead of four.  A tile is exactly three
    bodies -- first, mid, last -- so there is no single body; the wave's staging area shrinks to lds_stage_cap(4) entries
    (entries beyond it take .Lovf's global path), which is why only k <= 64 kNN passes run these bodies (launch_scan_space)."""
    global I8, I8_SPACE, NQT, L2C, ZZ, QB
    assert R in (2, 4) and nqt in (4, 8, 16) and (nqt == 16 or i8) and (not i8 or R == 4)
    assert l2c == (i8 and space == "l2")
    assert qbufs == 2 or (qbufs == 4 and i8 and nqt == 16)
    QB = qbufs
    try:
        return _generate(space, R, i8, nqt, l2c)
    finally:
        QB = 2


def _generate(space, R, i8, nqt, l2c):
    global I8, I8_SPACE, NQT, L2C, ZZ
    I8 = i8
    I8_SPACE = space if i8 else None
    NQT = nqt
    L2C = l2c
    ZZ = i8
    out = []
    a = out.append
    # ---- descriptors and per-workgroup state
    a("s_mov_b32 s80, %[xlo]")
    a("s_mov_b32 s81, %[xhi]")
    a("s_mov_b32 s82, %[wbytes]")
    a("s_mov_b32 s83, 0x00020000")
    a("s_mov_b32 s86, s82")
    a("s_mov_b32 s87, s83")
    a("s_mov_b32 s88, %[rnlo]")
    a("s_mov_b32 s89, %[rnhi]")
    if L2C:   # the offsets are read through the same descriptor, 8 x capacity bytes further on: no range to check against
        a("s_mov_b32 s90, -1")
        a("s_mov_b32 %[eo], %[eo0in]")
    else:
        a(f"s_movk_i32 s90, 0x{16 * MT * (8 if i8 else 4):x}")   # this wave's rows x 4 B (int8 shadow: pairs)
    a("s_mov_b32 s91, s83")
    a("s_mov_b32 %[tl], %[ntiles]")
    a("s_mov_b32 %[trow], %[row0]")
    a("s_mov_b32 %[wcnt], 0")
    if ZZ:
        # ---- prologue: Q chunks 0 and 1 -> LDS buffers 0 and 1 (what every even tile starts on: q_schedule), k-steps 0..R-1 ->
        # the ring.  A tile's first chunk does not toggle the buffers: reads start in buffer 0, transfers go to the other one.
        # Four buffers: chunks 0..3 -> buffers 0..3 (M0 reaches LDS addresses >= 64 KiB: tools/probe/dma_high_probe.hip).  Later
        # transfers go to buffers 0 and 1 only (gen_chunk).
        assert Q_BUFS == 2 and QB in (2, 4)   # (the xor toggle of sldw; three buffers would need a rotation here and in gen_chunk)
        a("v_mov_b32 %[ldr], %[lane16]")
        a("s_add_u32 %[sldw], %[wave2k], 0x8000")
        for c in range(QB):
            for _, _, const in dma_pieces():
                a(f"s_add_u32 m0, %[wave2k], 0x{c * CHUNK_BYTES + const:x}")
                a(f"s_mov_b32 %[st0], 0x{c * CHUNK_BYTES + const:x}")
                a("buffer_load_dwordx4 %[qvoff], %[qsrd], %[st0] offen lds")
        a(f"s_mov_b32 {XSTEP}, 0x400")             # the first tile walks upwards
        a(f"s_mov_b32 {QSTEP}, 0xffff8000")        # (.Ltile negates it)
        a(f"s_movk_i32 %[xso0], 0x{R * 1024:x}")   # the X cursors: k-step R of the first tile; they never restart (gen_chunk)
        a("s_add_u32 %[xso1], %[pb], %[xso0]")
    else:
        a("v_add_u32 %[ldr], 0x8000, %[lane16]")   # the first chunk moves it to buffer 0
        # ---- prologue: Q chunk 0 -> LDS buffer 0, k-steps 0..R-1 -> the ring
        a("s_mov_b32 %[sldw], %[wave2k]")          # buffer 0; the first chunk toggles it to buffer 1
        for _, _, const in dma_pieces():
            a(f"s_add_u32 m0, %[sldw], 0x{const:x}")
            a(f"s_movk_i32 %[st0], 0x{const:x}")
            a("buffer_load_dwordx4 %[qvoff], %[qsrd], %[st0] offen lds")
    for b in range(R):
        for m in range(MT):
            so = "0" if m == 0 else "%[pb]"
            off = f" offset:{b * 1024}" if b else ""
            a(f"buffer_load_dwordx4 {ring(b, m)}, %[lane16], {XCUR}, {so} offen{off}")
    if L2C:   # the first tile's offsets (every later tile's are fetched a tile ahead: gen_eo_loads)
        a("v_lshrrev_b32 %[e0], 1, %[rnvoff]")
        for m in range(MT):
            a(f"buffer_load_dwordx4 %[eo{m}], %[e0], {RNS}, %[eo] offen" + (f" offset:{64 * m}" if m else ""))
    a("s_waitcnt vmcnt(0)")
    a("s_waitcnt vmcnt(0) lgkmcnt(0)")   # counted waits below assume the steady-state issue pattern
    a("s_barrier")
    if i8 and space != "ip":   # the thresholds of this lane's query column in the 16 query tiles: constant for the whole launch
        for n in range(NQT):
            a(f"ds_read_b32 %[tq{n}], %[thra]" + (f" offset:{n * 64}" if n else ""))
        a("s_waitcnt lgkmcnt(0)")
    # ---- persistent loop over this workgroup's tiles
    a(".Ltile_%=:")
    a("s_cmp_gt_u32 %[tl], 1")           # next tile's descriptor (the last tile re-reads itself: harmless)
    a("s_cselect_b32 %[st0], %[xslo], 0")
    a("s_cselect_b32 %[cnt], %[xshi], 0")
    a("s_add_u32 s84, s80, %[st0]")
    a("s_addc_u32 s85, s81, %[cnt]")
    if ZZ:   # this tile's direction; the first chunk it stages (at its second position) is chunk 2, or nkc - 3 on the way down
        #      (four buffers: chunk 4, or nkc - 5, at its fourth position)
        a(f"s_sub_u32 {QSTEP}, 0, {QSTEP}")
        a(f"s_sub_u32 %[st0], %[qbytes], 0x{(QB + 1) * CHUNK_BYTES:x}")
        a(f"s_cmp_gt_i32 {QSTEP}, 0")
        a(f"s_cselect_b32 %[qcur], 0x{QB * CHUNK_BYTES:x}, %[st0]")
    else:
        a("s_mov_b32 %[qcur], %[qc1]")       # first chunk staged inside this tile's loop
        a(f"s_movk_i32 %[xso0], 0x{R * 1024:x}")
        a("s_add_u32 %[xso1], %[pb], %[xso0]")
    if QB != 4:   # (four buffers: a tile is three bodies, nb = 3)
        a("s_cmp_eq_u32 %[nb], 1")
        a("s_cbranch_scc1 .Lsingle_%=")
    out += body_lines(R, True, False, 0)
    a("s_sub_u32 %[cnt], %[nb], 2")
    a(".Lloop_%=:")
    a("s_cmp_eq_u32 %[cnt], 0")
    a("s_cbranch_scc1 .Llast_%=")
    out += body_lines(R, False, False, 100)
    a("s_sub_u32 %[cnt], %[cnt], 1")
    a("s_branch .Lloop_%=")
    a(".Llast_%=:")
    out += body_lines(R, False, True, 200)
    if QB != 4:
        a("s_branch .Ladmit_%=")
        a(".Lsingle_%=:")
        out += body_lines(R, True, True, 300)
    a(".Ladmit_%=:")
    if i8:
        a("s_setprio 0")   # (the pre-tests ran inside the last k-step: gen_pretest; .Lback<n> live there)
    else:
        out += gen_admission(space)
    a("s_mov_b32 s80, s84")
    a("s_mov_b32 s81, s85")
    a("s_add_u32 s88, s88, %[rnstride]")
    a("s_addc_u32 s89, s89, 0")
    if L2C:   # the pairs' base moved on by 8 bytes per row, the offsets' by 4: the distance shrinks by the difference
        a("s_lshr_b32 %[st0], %[rnstride], 1")
        a("s_sub_u32 %[eo], %[eo], %[st0]")
    a("s_add_u32 %[trow], %[trow], %[rowstride]")
    a("s_sub_u32 %[tl], %[tl], 1")
    a("s_cmp_lg_u32 %[tl], 0")
    a("s_cbranch_scc1 .Ltile_%=")
    # Kernel end.  The entries a wave staged in LDS are moved into the per-query candidate lists by the C++ tail of
    # filter_scan_asm_kernel (the workgroup's own scatter); the assembly only has to make sure everything it issued has
    # landed: ring / Q sets still in flight that nobody consumes, staged entries.  The entry count leaves through wcnt.
    a("s_waitcnt vmcnt(0) lgkmcnt(0)")
    if QB == 4 and Q4_SPARSE_BARRIERS:
        # The C++ tail reuses the Q buffers; no barrier follows a tile's last chunk position here.  Every wave of the
        # workgroup runs the same number of tiles, so all of them arrive.
        a("s_barrier")
    a("s_branch .Ldone_%=")
    if i8:   # one set per copy of the tile's last body (.Llast / .Lsingle): a stub returns into its copy
        out += gen_hit_stubs("c200") + (gen_hit_stubs("c300") if QB != 4 else [])
    else:
        out += gen_hit_stubs()
    out += gen_slow_fast() if i8 else gen_slow()
    a(".Ldone_%=:")

    ops_out, ops_in = [], []
    opc = "a" if i8 else "v"   # register class of the MFMA A / B operands
    for b in range(R):
        for m in range(MT):
            ops_out.append(f'[x{b * MT + m}] "=&{opc}"(xring[{b * MT + m}])')
    for i in range(QD):
        ops_out.append(f'[t{i}] "=&{opc}"(qt[{i}])')
    for j in range(4 * MT):
        ops_out.append(f'[r{j}] "=&v"(vr[{j}])')
    if (space == "l2" and not i8) or (i8 and space == "cosine"):
        for j in range(4 * MT):
            ops_out.append(f'[p{j}] "=&v"(vp[{j}])')
    if i8 and space == "ip":
        for j in range(4 * MT):
            ops_out.append(f'[s{j}] "=&v"(vs[{j}])')
    if L2C:
        for m in range(MT):
            ops_out.append(f'[eo{m}] "=&v"(veo[{m}])')
        ops_out.append('[eo] "=&s"(s_eo)')
    for j in range(4 * MT):
        ops_out.append(f'[u{j}] "=&v"(vu[{j}])')
    for j in range(13):
        ops_out.append(f'[e{j}] "=&v"(ve[{j}])')
    if i8:
        for n in range(NQT if space != "ip" else IP_TQ):
            ops_out.append(f'[tq{n}] "=&v"(vt[{n}])')
    ops_out += ['[ldr] "=&v"(ldr)', '[sldw] "=&s"(s_sldw)']
    for name in [f"xso{m}" for m in range(MT)] + ["qcur", "cnt", "st0", "tl", "trow", "sn64", "wcnt", "sacc0", "sacc1"]:
        ops_out.append(f'[{name}] "=&s"(s_{name})')
    ops_in += ['[qsrd] "s"(qsrd)', '[lane16] "v"(lane16)', '[qvoff] "v"(qvoff)', '[rnvoff] "v"(rnvoff)',
               '[thra] "v"(thra)', '[c16v] "v"(c16v)', '[crow] "v"(crow)', '[stg] "v"(stg)',
               '[xlo] "s"(xlo)', '[xhi] "s"(xhi)', '[wbytes] "s"(wbytes)', '[xslo] "s"(xslo)', '[xshi] "s"(xshi)',
               '[rnlo] "s"(rnlo)', '[rnhi] "s"(rnhi)', '[rnstride] "s"(rnstride)',
               '[row0] "s"(row0)', '[rowstride] "s"(rowstride)', '[ntiles] "s"(ntiles)',
               '[pb] "s"(pb)', '[qbytes] "s"(qbytes)', '[nb] "s"(nb)', '[qcur0] "s"(qcur0)', '[qc1] "s"(qc1)',
               '[wtype] "s"(wtype)', '[wgbu] "s"(wgbu)', '[wgbr] "s"(wgbr)', '[wgbq] "s"(wgbq)', '[wgcp] "s"(wgcp)',
               '[ovfb] "s"(ovfb)']
    if (space == "l2" and not i8) or (i8 and space == "cosine"):
        ops_in.append('[k1] "s"(k1)')
    if L2C:
        ops_in += ['[sqc] "s"(sqc)', '[kec] "s"(kec)', '[krc] "s"(krc)']
    ops_in.append('[wave2k] "s"(wave2k)')
    if L2C:
        ops_in.append('[eo0in] "s"(eo0)')
    clobbers = ['"memory"', '"scc"', '"vcc"', '"m0"'] + [f'"s{i}"' for i in range(60, 94)] + (
        [f'"v{i}"' for i in range(VA_BASE, VA_BASE + 64 * MT)] if i8 else [f'"a{i}"' for i in range(64 * MT)])

    text = ["// GENERATED by tools/gen_scan_asm.py -- do not edit.",
            f"// filter scan body: space {space}, NW={NW} waves x {16 * MT} rows, ring R={R} k-steps, B fragments read {QD} ahead"
            f", X loads non-temporal{', progress-based wave priority' if i8 else ''}, Q staged by LDS-DMA{', k-chunks zig-zag' if ZZ else ''}"
            f"{', int8 shadow (v_mfma_i32_16x16x64_i8)' if i8 else ''}{', accumulators in ArchVGPRs' if i8 else ''}"
            f"{f', {QB} Q buffers ({Q4_NKC} chunks)' if QB != 2 else ''}.",
            "asm volatile("]
    for ln in out:
        text.append(f'    "{ln}\\n\\t"')
    text.append("    : " + ",\n      ".join(ops_out))
    text.append("    : " + ",\n      ".join(ops_in))
    text.append("    : " + ", ".join(clobbers) + ");")
    return "\n".join(text) + "\n"


def default_i8_body(space):
    """The int8 body the library runs for a full pass in `space`: scan_asm_<space>_i8_va.inc; l2: the 16-tile l2c body,
    scan_asm_l2_i8_va_c_nqt16.inc."""
    return generate(space, 4, i8=True, nqt=16, l2c=space == "l2")


# ---------------------------------------------------------------------------------------------------------------------
# What gets generated: (file name, dispatch condition on filter_scan_asm_kernel's template arguments <SPACE, R, I8, NQT, QB>,
# thunk that returns the text)
def cond(space, r, i8, nqt, qb=2):
    return f"SPACE == {SPACES[space]} && R == {r} && {'I8' if i8 else '!I8'} && NQT == {nqt} && QB == {qb}"


def q4_body(space):
    """The four-buffer int8 body of a full pass in `space` (an image of Q4_NKC chunks)."""
    return generate(space, 4, i8=True, nqt=16, l2c=space == "l2", qbufs=4)


def entries():
    E = []
    for sp in SPACES:   # the int8 bodies, 16 / 8 / 4 query tiles (passes of 256 / <= 128 / <= 64 queries); l2: l2c
        for nqt in (16, 8, 4):
            name = (f"scan_asm_l2_i8_va_c_nqt{nqt}.inc" if sp == "l2" else
                    f"scan_asm_{sp}_i8_va{'' if nqt == 16 else f'_nqt{nqt}'}.inc")
            E.append((name, cond(sp, 4, True, nqt), lambda sp=sp, nqt=nqt: generate(sp, 4, True, nqt, sp == "l2")))
    for sp in SPACES:   # the four-buffer int8 bodies: full passes over an image of Q4_NKC chunks (k <= 64 kNN passes)
        name = "scan_asm_l2_i8_va_c_nqt16_q4.inc" if sp == "l2" else f"scan_asm_{sp}_i8_va_q4.inc"
        E.append((name, cond(sp, 4, True, 16, 4), lambda sp=sp: q4_body(sp)))
    for sp in SPACES:   # bf16 bodies of an index that keeps a bf16 shadow: ring of 4 k-steps (2: odd chunk counts)
        for r in (4, 2):
            E.append((f"scan_asm_{sp}_nw8_r{r}_nt_dma.inc", cond(sp, r, False, 16), lambda sp=sp, r=r: generate(sp, r)))
    return E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default=str(Path(__file__).resolve().parents[1] / "mlvectordb_amd" / "csrc"))
    ap.add_argument("--list", action="store_true", help="print the generated file names and exit")
    args = ap.parse_args()
    E = entries()
    names = [e[0] for e in E] + ["scan_asm_dispatch.inc", "scan_asm_consts.inc"]
    if args.list:
        print(" ".join(names))
        return
    out = Path(args.outdir)
    for name, _, thunk in E:
        (out / name).write_text(thunk())
    disp = ["// GENERATED by tools/gen_scan_asm.py -- do not edit.  Body of filter_scan_asm_kernel<SPACE, R, I8, NQT, QB>."]
    for i, (name, c, _) in enumerate(E):
        disp.append(("if" if i == 0 else "} else if") + f" constexpr ({c}) {{")
        disp.append(f'#include "{name}"')
    disp.append("} else {")
    disp.append('    static_assert(SPACE < 0, "configuration not generated: see entries() in tools/gen_scan_asm.py");')
    disp.append("}")
    (out / "scan_asm_dispatch.inc").write_text("\n".join(disp) + "\n")
    (out / "scan_asm_consts.inc").write_text(
        "// GENERATED by tools/gen_scan_asm.py -- do not edit.\n"
        f"constexpr int kAsmWgCap = {WG_CAP};\n"
        f"constexpr int kAsmQBufs = {Q_BUFS};  // Q chunk buffers in LDS\n"
        f"constexpr int kAsmStageCap = {lds_stage_cap()};  // entries per wave staged in LDS\n"
        f"constexpr int kAsmQ4Chunks = {Q4_NKC};  // the four-buffer bodies: the image's chunk count they are written for\n"
        f"constexpr int kAsmQ4StageCap = {lds_stage_cap(4)};  // ... and their staging area, entries per wave\n")
    print("wrote", len(names), "files to", args.outdir)


if __name__ == "__main__":
    main()
