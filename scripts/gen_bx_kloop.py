#!/usr/bin/env python3
"""Generator of the hand-scheduled K loop of gemm256_bx_kernel<6, true> (vivit_amd/csrc/gemm_tile256_bx.hip) as an inline-asm block.

    python scripts/gen_bx_kloop.py            # writes vivit_amd/csrc/bx_kloop_asm.inc (committed: the build never runs this)

VERDICT r03-r05 asked for the loop body in assembly: fixed register map, the global -> LDS requests of a K tile placed by
hand between the MFMAs.  The block runs `ntiles` K tiles (16 k each) of the pipeline the C++ loop runs (gemm_tile256_bx.hip,
"Pipeline (tile t lives in stage t % 3)") and is entered / left in that loop's invariant:

    entry: tile t has landed in stage st and is published (every wave is past the barrier that followed its wait), the
           requests of tile t + 1 are in flight, nothing of tile t is in registers;
    exit : the same for t + ntiles; the accumulator tiles are updated (st and the request pointers are inputs: the caller
           advances its copies by ntiles).

Arithmetic contract (bit-identical to the C++ loop): every accumulator tile sees, per K tile, the six partial products in the
order (lo hi), (hi lo), (mid mid), (mid hi), (hi mid), (hi hi) of (A piece, B piece), two per instruction -- mfma_row of the C++
loop, see Geometry16 below -- and the K tiles in ascending order.  Only the order BETWEEN accumulators and the placement of
memory instructions differ.

Three K tiles per trip, the stage registers taking their roles by renaming (no rotation moves).  The twelve requests of a tile
take a scalar base each (s[40:63], steps in s[64:67]) and ONE per-lane 32-bit offset: `global_load_lds_dwordx4 v, s[..]`.

(Until round 6 this script also generated the 32 x 32 x 16 form of the block and the experiment and timing-only blocks of the
attribution builds.  They were removed after their measurements: profiles/r06_bx_attribution*.log, profiles/r06_bx16_timeline*.log,
profiles/r06_syrk_ab_s16.log)
"""
import os

BX_PIECE = 8 * 1024
BX_OPER = 3 * BX_PIECE
BX_STAGE = 2 * BX_OPER

S_CUR, S_NXT, S_NN, S_DMA, S_CNT, S_TMP = "s84", "s85", "s86", "s87", "s88", "s89"
CLOBBER_S = list(range(84, 90))
# the twelve request streams as SGPR base pairs s[40:63] + ONE per-lane 32-bit offset (global_load_lds v, s[..]); steps in s[64:67]
SADDR_BASE, SADDR_STEP = 40, 64
CLOBBER_S_SADDR = list(range(40, 68))
UNROLL = 3                       # K tiles per trip
BARRIER_GAP = 96                 # the mid-tile wait + barrier: in front of the MFMAs of row tile 4
REQ_GAPS = [100, 104, 108, 112, 116, 124, 128, 132, 136, 140, 148, 152]   # the MFMA slot BEFORE which request r is issued


class Emitter:
    def __init__(self):
        self.lines = []
        self.lgkm = []      # names of outstanding ds_reads, oldest first (the LDS returns data in order)

    def raw(self, s):
        self.lines.append(s)

    def ds_read(self, name, dst, addr, offset):
        self.raw(f"ds_read_b128 {dst}, {addr} offset:{offset}")
        self.lgkm.append(name)

    def need(self, names):
        """s_waitcnt lgkmcnt(N) so that every fragment in `names` has arrived (N = reads issued behind the youngest needed)."""
        idx = [self.lgkm.index(n) for n in names if n in self.lgkm]
        if not idx:
            return
        keep = min(len(self.lgkm) - 1 - max(idx), 15)   # (4-bit counter: waiting for more than needed is always safe)
        self.raw(f"s_waitcnt lgkmcnt({keep})")
        del self.lgkm[: max(idx) + 1]


# ------------------------------------------------------------------------------------------------------------------------------
# The v_mfma_f32_16x16x32_bf16 form (gemm_tile256_bx.hip "S16").  One instruction adds TWO partial products: its K = 32 is the tile's 16 k
# twice, with a different pair of pieces each time (the lanes of k blocks 0, 1 read one piece, those of blocks 2, 3 the other -- the
# per-lane piece offset is folded into the fragment address the C++ side passes in).  Per 16 x 16 accumulator (rt, ct) and K tile
# three instructions in this order (smallest terms first; mfma_row of the C++ loop):
#     m = 0: A[a2 | a0] x B[b0 | b2]      m = 1: A[a1 | a1] x B[b1 | b0]      m = 2: A[a0 | a0] x B[b1 | b0]
# The wave's 128 x 128 are 8 x 8 such accumulators: a[16 (4 (rt / 2) + ct / 2) + 4 (2 (rt % 2) + ct % 2) ..+3] (acc[i][j][q] of the
# C++ side, pinned by "+{a[..]}" constraints).  Per wave and K tile: 192 MFMAs (16 cycles each), 40 ds_read_b128 (3 A fragments per
# row tile, 2 B fragments per column tile; the 16 B fragments stay in registers for the tile), 12 requests.
# Register map (base 128): B fragments 64, A sets X / Y 12 each, 8 fragment addresses (A now x 3, A next x 3, B next x 2), the lane
# offset of the requests, 24 scratch registers for the request bases at entry.
class Geometry16:
    nw, nj, nu = 4, 4, 2
    nmfma = 192
    nacc_operands = 64

    def __init__(self):
        v0 = 128
        self.vb0 = v0
        self.vax = v0 + 64
        self.vay = self.vax + 12
        self.vaddr = self.vay + 12       # 8 address registers + lane offset
        self.vp0 = self.vaddr + 10      # (64-bit pairs: even register numbers)
        self.npair = 12
        self.clobber_v = list(range(v0, self.vp0 + 2 * self.npair))
        assert self.clobber_v[-1] < 256
        k = self.nacc_operands
        self.cofs_a = [f"%{k + c}" for c in range(3)]
        self.cofs_b = [f"%{k + 3 + d}" for d in range(2)]
        k += 5
        self.src = {}
        for op in "AB":
            for u in range(self.nu):
                self.src[(op, u)] = f"%{k}"
                k += 1
        self.stride = {"A": f"%{k}", "B": f"%{k + 1}"}
        self.step = {"A": f"%{k + 2}", "B": f"%{k + 3}"}
        self.lds0, self.st, self.nt, self.grp = f"%{k + 4}", f"%{k + 5}", f"%{k + 6}", f"%{k + 7}"
        self.noperands = k + 8

    @staticmethod
    def acc(rt, ct):
        k = 16 * (4 * (rt >> 1) + (ct >> 1)) + 4 * (2 * (rt & 1) + (ct & 1))
        return f"a[{k}:{k + 3}]"

    def vb(self, ct, d):
        k = self.vb0 + 4 * (2 * ct + d)
        return f"v[{k}:{k + 3}]"

    def va(self, s, c):
        k = (self.vax if s == 0 else self.vay) + 4 * c
        return f"v[{k}:{k + 3}]"

    def v_ac(self, c):      # address of this lane's A fragments of combination c, current tile
        return f"v{self.vaddr + c}"

    def v_an(self, c):      # ... next tile
        return f"v{self.vaddr + 3 + c}"

    def v_bn(self, d):      # B fragments of combination d, next tile
        return f"v{self.vaddr + 6 + d}"

    @property
    def v_off(self):
        return f"v{self.vaddr + 8}"

    def pair(self, op, u, pc):
        k = self.vp0 + 2 * ((0 if op == "A" else 3 * self.nu) + 3 * u + pc)
        return f"v[{k}:{k + 1}]"

    def sbase(self, op, u, pc):
        return SADDR_BASE + 2 * ((0 if op == "A" else 3 * self.nu) + 3 * u + pc)

    def requests(self):
        """The requests of one K tile in the C++ order: part q = (block u = q / 2, operand q % 2), three pieces each."""
        out = []
        for q in range(2 * self.nu):
            u, op = q >> 1, "AB"[q & 1]
            for pc in range(3):
                out.append((op, u, pc))
        return out

    @staticmethod
    def tile_ofs(t):        # byte offset of 16-row tile t of the wave inside a piece
        return (t >> 1) * 1024 + (t & 1) * 256


def stream16():
    """(rt, ct, m) of the 192 MFMAs of a K tile: row tile by row tile, product by product over the eight column tiles, so that an
    accumulator comes back every 8th instruction (walking the columns of row tiles 0 and 7 in pairs -- an accumulator every 2nd
    instruction -- cost ~130 cycles per K tile: the dependent instruction waits for the result)."""
    return [(rt, ct, m) for rt in range(8) for m in range(3) for ct in range(8)]


def next_b_order():
    """Order in which a tile reads the NEXT tile's B fragments (= the order of the reads at entry)."""
    return [(ct, 0) for ct in range(8)] + [(ct, 1) for ct in range(8)]


def one_tile16(e, G, S_CUR, S_NXT, S_NN):
    """One K tile: the MFMA stream with its fillers.  M0 of a request is written one gap ahead of it: the MFMA in between is the
    wait state the LDS-DMA needs behind a write of M0 (instead of an s_nop in front of the request)."""
    reqs = G.requests()
    assert len(REQ_GAPS) == len(reqs)
    for c in range(3):
        e.raw(f"v_add_u32 {G.v_ac(c)}, {S_CUR}, {G.cofs_a[c]}")
    e.raw(f"s_add_u32 {S_DMA}, {G.lds0}, {S_NN}")
    stream = stream16()
    N = G.nmfma
    assert len(stream) == N
    fillers = {g: [] for g in range(N + 2)}
    for rt in range(1, 8):      # A fragments of row tile rt behind the first MFMAs of row tile rt - 1
        fillers[24 * (rt - 1)] += [("ds", f"A{rt}{c}", G.va(rt & 1, c), G.v_ac(c), G.tile_ofs(rt)) for c in range(3)]
    fillers[BARRIER_GAP] += [("barrier",)]
    # addresses of the next tile's fragments: computed behind the barrier, used from row tile 7 on
    fillers[BARRIER_GAP + 1] += [("valu", f"v_add_u32 {G.v_an(c)}, {S_NXT}, {G.cofs_a[c]}") for c in range(3)]
    fillers[BARRIER_GAP + 2] += [("valu", f"v_add_u32 {G.v_bn(d)}, {S_NXT}, {G.cofs_b[d]}") for d in range(2)]
    fillers[24 * 7] += [("ds", f"N0{c}", G.va(0, c), G.v_an(c), 0) for c in range(3)]
    # row tile 7: the [b0 | b2] fragments are dead behind its first eight MFMAs, the [b1 | b0] fragment of column ct behind the
    # last MFMA of that column -- the next tile's take their registers, one read per gap
    fillers[24 * 7 + 8] += [("ds", f"NB{ct}0", G.vb(ct, 0), G.v_bn(0), G.tile_ofs(ct)) for ct in range(8)]
    for ct in range(8):
        fillers[24 * 7 + 16 + ct + 1] += [("ds", f"NB{ct}1", G.vb(ct, 1), G.v_bn(1), G.tile_ofs(ct))]
    for r, g in enumerate(REQ_GAPS):
        assert BARRIER_GAP <= g <= N, "requests overwrite the stage of tile t - 1: only behind the mid-tile barrier"
        assert r == 0 or g - 1 > REQ_GAPS[r - 1], "M0 of a request is written before the previous request has been issued"
        fillers[g - 1].append(("m0", r))
        fillers[g].append(("req", r))
        fillers[g + 1].append(("reqstep", r))
    # one fragment read per gap (16 cycles): the overflow moves to the following gaps (never across the end of the tile)
    for g in range(N):
        reads = [f for f in fillers[g] if f[0] == "ds"]
        if len(reads) > 1:
            move = reads[1:]
            fillers[g] = [f for f in fillers[g] if f not in move]
            fillers[g + 1] = move + fillers[g + 1]

    def emit_fillers(g):
        for f in fillers[g]:
            if f[0] == "ds":
                e.ds_read(f[1], f[2], f[3], f[4])
            elif f[0] == "valu":
                e.raw(f[1])
            elif f[0] == "barrier":
                e.raw("s_waitcnt vmcnt(0)")          # this wave's share of tile t + 1 has landed
                e.raw("s_barrier")                   # publishes tile t + 1; every wave is past tile t - 1
            elif f[0] == "m0":
                op, u, pc = reqs[f[1]]
                e.raw(f"s_add_u32 m0, {S_DMA}, {(BX_OPER if op == 'B' else 0) + pc * BX_PIECE + G.nw * u * 1024}")
            elif f[0] == "req":
                b = G.sbase(*reqs[f[1]])
                e.raw(f"global_load_lds_dwordx4 {G.v_off}, s[{b}:{b + 1}]")
            elif f[0] == "reqstep":
                op, u, pc = reqs[f[1]]
                b = G.sbase(op, u, pc)
                st_ = SADDR_STEP + (0 if op == "A" else 2)
                e.raw(f"s_add_u32 s{b}, s{b}, s{st_}")
                e.raw(f"s_addc_u32 s{b + 1}, s{b + 1}, s{st_ + 1}")

    e.lgkm = [f"A0{c}" for c in range(3)] + [f"B{ct}{d}" for ct, d in next_b_order()]
    for g, (rt, ct, m) in enumerate(stream):
        emit_fillers(g)
        d = 0 if m == 0 else 1
        e.need([f"A{rt}{m}", f"B{ct}{d}"])
        e.raw(f"v_mfma_f32_16x16x32_bf16 {G.acc(rt, ct)}, {G.va(rt & 1, m)}, {G.vb(ct, d)}, {G.acc(rt, ct)}")
    emit_fillers(N)
    emit_fillers(N + 1)
    want = [f"N0{c}" for c in range(3)] + [f"NB{ct}{d}" for ct, d in next_b_order()]
    assert e.lgkm == want, e.lgkm


def gen16():
    G = Geometry16()
    e = Emitter()
    e.raw("; ---- entry: stage offsets of tiles t, t + 1, t + 2 from st; scalar bases of the twelve request streams")
    e.raw(f"s_mul_i32 {S_CUR}, {G.st}, {BX_STAGE}")
    e.raw(f"s_add_u32 {S_NXT}, {S_CUR}, {BX_STAGE}")
    e.raw(f"s_cmp_eq_u32 {G.st}, 2")
    e.raw(f"s_cselect_b32 {S_NXT}, 0, {S_NXT}")
    e.raw(f"s_add_u32 {S_NN}, {S_NXT}, {BX_STAGE}")
    e.raw(f"s_cmp_eq_u32 {S_NXT}, {2 * BX_STAGE}")
    e.raw(f"s_cselect_b32 {S_NN}, 0, {S_NN}")
    e.raw(f"s_mov_b32 {S_CNT}, {G.nt}")
    for op in "AB":
        for u in range(G.nu):
            e.raw(f"v_lshl_add_u64 {G.pair(op, u, 0)}, {G.src[(op, u)]}, 0, 0")
            e.raw(f"v_lshl_add_u64 {G.pair(op, u, 1)}, {G.stride[op]}, 0, {G.src[(op, u)]}")
            e.raw(f"v_lshl_add_u64 {G.pair(op, u, 2)}, {G.stride[op]}, 1, {G.src[(op, u)]}")
    first = G.pair("A", 0, 0)
    for op in "AB":
        for u in range(G.nu):
            for pc in range(3):
                b, vp = G.sbase(op, u, pc), G.pair(op, u, pc)
                lo = int(vp[2:].split(":")[0])
                e.raw(f"v_readfirstlane_b32 s{b}, v{lo}")
                e.raw(f"v_readfirstlane_b32 s{b + 1}, v{lo + 1}")
    lo0 = int(first[2:].split(":")[0])
    e.raw(f"v_readfirstlane_b32 {S_TMP}, v{lo0}")
    e.raw("s_nop 4")                                   # VALU-written SGPR -> read by VALU / VMEM
    e.raw(f"v_sub_u32 {G.v_off}, v{lo0}, {S_TMP}")
    e.raw(f"s_mov_b64 s[{SADDR_STEP}:{SADDR_STEP + 1}], {G.step['A']}")
    e.raw(f"s_mov_b64 s[{SADDR_STEP + 2}:{SADDR_STEP + 3}], {G.step['B']}")
    # fragments of tile t in the order in which a tile requests the NEXT tile's (one model of the LDS return queue for every tile)
    for c in range(3):
        e.raw(f"v_add_u32 {G.v_an(c)}, {S_CUR}, {G.cofs_a[c]}")
    for d in range(2):
        e.raw(f"v_add_u32 {G.v_bn(d)}, {S_CUR}, {G.cofs_b[d]}")
    for c in range(3):
        e.ds_read(f"A0{c}", G.va(0, c), G.v_an(c), 0)
    for ct, d in next_b_order():
        e.ds_read(f"B{ct}{d}", G.vb(ct, d), G.v_bn(d), G.tile_ofs(ct))
    label = "BXK_G0_%="
    e.raw(f"{label}:")
    regs = [S_CUR, S_NXT, S_NN]
    for k in range(UNROLL):
        one_tile16(e, G, regs[k % 3], regs[(k + 1) % 3], regs[(k + 2) % 3])
    e.raw(f"s_sub_u32 {S_CNT}, {S_CNT}, {UNROLL}")
    e.raw(f"s_cmp_lg_u32 {S_CNT}, 0")
    e.raw(f"s_cbranch_scc1 {label}")
    e.raw("; ---- exit: nothing of the next tile is needed in registers (the C++ side re-reads its fragments)")
    e.raw("s_waitcnt lgkmcnt(0)")
    return e.lines, G


def acc_operands16():
    """The 64 accumulators of the C++ side (acc[i][j][q]) pinned to the AGPRs the block names."""
    ops = []
    for i in range(4):
        for j in range(4):
            for q in range(4):
                k = 16 * (4 * i + j) + 4 * q
                ops.append(f'"+{{a[{k}:{k + 3}]}}"(ACC[{i}][{j}][{q}])')
    return ", ".join(ops)


def render(lines, G, name):
    clob = ", ".join([f'"v{k}"' for k in G.clobber_v] + [f'"s{k}"' for k in CLOBBER_S + CLOBBER_S_SADDR] + ['"scc"', '"memory"'])
    # (m0 is written too: clang reserves it and refuses it as a clobber; hipcc keeps nothing live in m0 across an asm statement)
    return (f"#define {name}_TEXT \\\n" + " \\\n".join(f'  "{l}\\n\\t"' for l in lines) + f"\n#define {name}_CLOBBERS {clob}\n"
            f"#define {name}_UNROLL {UNROLL}\n#define {name}_ACC(ACC) {acc_operands16()}\n")


HEADER = """// GENERATED by scripts/gen_bx_kloop.py -- do not edit; see that script for the register map, the pipeline invariant at
// entry / exit and the arithmetic contract (bit-identical to the C++ K loop of gemm256_bx_kernel<6>).
"""

PRODUCT_BLOCKS = ("BX_KLOOP_ASM",)


def block_text(name):
    lines, G = gen16()
    return render(lines, G, name), lines, G


def product_text():
    """The committed file csrc/bx_kloop_asm.inc."""
    return HEADER + "".join(block_text(name)[0] for name in PRODUCT_BLOCKS)


def main():
    path = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vivit_amd", "csrc", "bx_kloop_asm.inc"))
    with open(path, "w") as f:
        f.write(product_text())
    print("wrote", path)


if __name__ == "__main__":
    main()
