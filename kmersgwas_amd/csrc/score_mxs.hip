// score_mxs.hip — the block-scaled filter of score_mx.hip in its OPERAND-STREAMING form, for shapes whose slice operands
// do not fit the LDS in one piece (2048 samples x 201 columns: 520 KB; 1135 x 101: 161 KB). Same contract, same operand
// bytes, same accumulators, same test and the same survivors' bitmap as mx_kernel (see there for the sample <-> k maps,
// the FP4 / FP6 slice grids and the bound; calculate_kmer_score: src/kmers_multiple_databases.cpp:327-363) - what changes
// is where the operands are while a row is multiplied:
//
//   mx_kernel   all steps of CT column tiles resident in LDS; a shape with more columns than fit becomes several "LDS
//               groups", and EVERY row is loaded, expanded to FP4 operands and tested once per group (five times at
//               2048 x 201, 15 column tiles for the 12.6 the columns need, >= 1.86 x the algorithmic HBM traffic).
//   mxs_kernel  the waves of a block keep the accumulators of ALL column tiles of an operand group (up to 14) for their row tiles
//               and walk the sample axis ONCE: the operands of one step (128 samples x all column tiles: 2560 B per tile, 35 KB
//               for 14) stream through a ring of LDS slots, fetched with `global_load_lds_dwordx4` (global -> LDS, no registers)
//               three steps ahead of their use by all waves of the block together, one `s_barrier` per step. Every row is
//               loaded and expanded once; the operands (L2-resident: 560 KB per operand group) cross the L2 -> LDS path once
//               per block pass (256 rows). No limit on the number of samples: nothing but one step's operands is in LDS.
//
//   ring protocol, step s (block-wide step counter, continuing across the block's passes; RING slots, AHEAD = RING - 1):
//     top of step s:  s_waitcnt vmcnt(N)   this wave's part of slab s + 1 (issued in step s + 1 - AHEAD) has landed - N = the
//                                          constant number of younger operations (see WAIT_N): they stay in flight
//                     s_barrier            (B_s) every wave's part has; every wave is through step s - 1's operand reads
//                     issue slab s + AHEAD into slot (s + AHEAD) % RING = the slot step s - 1 read; then RT row requests / fillers
//     during step s:  operand reads of step s (slot s % RING) and, in its last unit, of step s + 1's first unit
//   Every vector-memory operation of the main loop - the slabs, the row pieces (LDS-DMA into a per-wave staging area, picked up
//   with ds_read_b128), the fillers - is issued by inline assembly: the compiler would otherwise wait for every LDS-DMA in
//   flight before the next ds_read that may alias it, and for ALL outstanding operations where it first uses a loaded value.
//   It neither sees these transfers nor counts them, so the waits above are explicit, and every such statement carries a
//   "memory" clobber (the ring changes behind the compiler's back).
//
// Shapes (template): CT column tiles per wave, RT row tiles per wave, NG column groups among the waves of a block (a group =
// TH / 64 / NG waves with their own rows; the groups of a block share rows and split the column tiles, each with its own ones
// column), TH threads, RING slots (4 where they fit the LDS, else 3).
//   < 7, 4, 2, 512>  2048 x 201 (the default above 7 tiles): waves w and w + 4 work on the same 64 rows, 7 tiles each (14 for 12.6)
//   < 7, 4, 1, 512>  up to 7 tiles (1135 x 101: 9 steps x 7 tiles instead of two LDS groups of 4): eight waves of 64 rows
//   <13, 2, 1, 512>  KGWAS_MXS_FORM=1: 13 tiles, eight waves of 32 rows (104 accumulator registers; twice the LDS reads per MFMA)
//   <13, 4, 1, 256>  KGWAS_MXS_FORM=2: one wave per SIMD with the 512-register budget, 64 rows x 13 tiles (208)
//
// Measured (round 5): at 2048 x 201 and 1135 x 101 the default shapes run within +-2 % of the resident plan's
// launches (40.4 against 40.3 ms, 13.3 against 13.4 ms per 100 M rows) with the rows read from HBM once instead of once per LDS
// group; the 13-tile shapes are slower (46.7 / 46.8 ms). What the form adds is reach: 6000 accessions x 101 columns go through
// the filter (31.7 ms per 20 M rows; the exact scorer, the only path such a panel had: 4.7 s).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "filter_common.h"

// timing experiments only (wrong results): 1 no tests (acts in filter_common.h), 8 no row loads, 16 no operand DMA, 64 no
// barriers, 128 every row load hits the L2
#ifndef KGWAS_MXS_ABLATE
#define KGWAS_MXS_ABLATE 0
#endif

#ifndef KGWAS_MXS_PROF  // experiments: cycle counters of wave 0 of every block (sync waits, steps, epilogues) summed into mxs_prof[]
#define KGWAS_MXS_PROF 0
#endif

namespace kgwas {

#if KGWAS_MXS_PROF
__device__ unsigned long long mxs_prof[8];  // [0] cycles in step_sync, [1] cycles in steps (incl. sync), [2] epilogue cycles, [3] steps, [4] passes, [5] whole-kernel cycles of wave 0
extern "C" int kgwas_debug_mxs_prof(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mxs_prof), sizeof(mxs_prof)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(mxs_prof), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif

namespace {
constexpr uint32_t MXS_SB = mx_step_bytes(2, 0);  // FP6 slice + FP4 slice of one (step, column tile): 2560 B
}  // namespace

template <int CT, int RT, int NG, int TH, int RING>
__global__ void __launch_bounds__(TH) mxs_kernel(MxArgs a, uint32_t rows_per_block, uint32_t n_rowblocks) {
    extern __shared__ uint4 mslds[];  // ring[3][CTA x 2560], colc[3][SLOTS_ALL] (alpha, -, column index), per-wave row-term exchange
    constexpr uint32_t MXS_RING = RING;        // ring slots
    constexpr uint32_t MXS_AHEAD = RING - 1u;  // a slab is requested this many steps before the step that multiplies with it
    constexpr int CTA = CT * NG;          // column tiles of the block's operand slab
    constexpr int SLOTS = CT * 16;        // operand columns of a column group
    constexpr int SLOTS_ALL = CTA * 16;
    constexpr int WPG = TH / 64 / NG;     // waves per column group
    constexpr uint32_t SLAB = CTA * MXS_SB;
    constexpr uint32_t SLOT = (SLAB + 1023u) / 1024u * 1024u;  // ring slot (the last transfer of a slab may run up to 1 KB past it)
    typedef MxOperands<CT, 2, 4> Ops;  // two slices, FP6 + FP4
    static_assert(RT == 2 || RT == 4, "row tiles per wave");
    // every (row block, operand group) pair is a block
    const FilterBlock fb = filter_block(a.n_lgroups, a.n_lgroups > 1);
    const uint32_t rb = fb.rb, lg = fb.lg0;
    if (rb >= n_rowblocks) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t grp = wave / WPG, wig = wave % WPG;
    const uint32_t kb = lane >> 4, m = lane & 15u;
    const uint32_t n_steps = 4u * a.n_full + a.n_quarter;
    char* lds = reinterpret_cast<char*>(mslds);
    float* colc = reinterpret_cast<float*>(lds + MXS_RING * SLOT);
    const int* colp = reinterpret_cast<const int*>(colc + 2 * SLOTS_ALL) + grp * SLOTS;
    float* wscr = colc + 3 * SLOTS_ALL + wave * (RT * 48u);  // wave-private: RT*16 x N1, RT*16 x (sqrt(d), E)
    const uint32_t rows_per_pass = WPG * (RT * 16u);
    const uint64_t blk_row0 = (uint64_t)rb * rows_per_block;
    const char* rows_base = reinterpret_cast<const char*>(a.src.base);
    const uint32_t avail_b = a.src.avail_dw * 4u;
    const int sc0 = (int)a.scale0;
    uint32_t tested_local = 0;

    // passes of this block: the same for all its waves (they meet at a barrier every step)
    uint32_t n_passes;
    {
        const uint64_t left = a.n_rows - blk_row0;
        const uint32_t rows = left < rows_per_block ? (uint32_t)left : rows_per_block;
        n_passes = (rows + rows_per_pass - 1u) / rows_per_pass;
    }

    // ---- the operand stream: slab (step) -> ring slot, 16-byte units, unit u = i * TH + thread of round i
    const uint8_t* slab_src = a.Bq + (size_t)lg * n_steps * SLAB;
    const uint32_t lds_ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
    constexpr uint32_t N_UNITS = SLAB / 16u;
    constexpr uint32_t ROUNDS = (N_UNITS + TH - 1u) / TH;
    const uint32_t voff = lane * 16u;
    uint32_t dma_step = 0, dma_slot = 0;  // the next slab to fetch and where it goes
    // No branches in here (a branch in the step splits the main loop's body, see mx_kernel): a wave whose units of the last
    // round lie beyond the slab fetches its units of round 0 again, and the one wave that straddles the slab's end reads on
    // into the next slab (the buffer ends with 1 KB of padding) and writes into the slot's own padding (SLOT is SLAB rounded
    // up to whole KB).
    auto issue_slab = [&]() {
        if (KGWAS_MXS_ABLATE & 16) return;
        const uint8_t* src = slab_src + (size_t)dma_step * SLAB;
        const uint32_t dst = lds_ring + dma_slot * SLOT;
#pragma unroll
        for (uint32_t i = 0; i < ROUNDS; i++) {
            uint32_t ub = i * TH + wave * 64u;  // first unit of this wave's instruction
            if ((i + 1u) * TH > N_UNITS) ub = ub < N_UNITS ? ub : wave * 64u;  // (a scalar select)
            const uint32_t m0v = dst + ub * 16u;
            const uint8_t* sb = src + (size_t)ub * 16u;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(voff), "s"(sb) : "memory");
        }
        dma_step = dma_step + 1u == n_steps ? 0u : dma_step + 1u;
        dma_slot = dma_slot + 1u == MXS_RING ? 0u : dma_slot + 1u;
    };
    // The vector-memory sequence of EVERY step is [ROUNDS slab transfers][RT row operations] - the row operations being the
    // wave's row loads of the next 512-sample group in the one step per group that issues them, and RT four-byte LDS-DMA
    // fillers (a hot line into a scratch area nobody reads) in every other step. Loads complete in order and `s_waitcnt vmcnt`
    // takes an immediate: with a uniform sequence "slab s + 1 has landed" is the constant vmcnt(WAIT_N) at the top of step s,
    // however many younger operations - the next slabs, the row loads - are still in flight. A row load issued in step s must
    // then have landed by the top of step s + MXS_AHEAD (it is older than the slab requested in step s + 1, which is waited
    // for there): three steps, ~7000 cycles, against ~4000 of HBM latency. (With vmcnt(0) every step - the first version -
    // every wave waited out its row loads' HBM latency one step after issuing them, and the block with it: +13 % kernel time.)
    constexpr uint32_t WAIT_N = RT + (MXS_AHEAD - 2u) * (ROUNDS + RT);
    static_assert(MXS_AHEAD >= 2u && WAIT_N < 64u, "vmcnt is a 6-bit immediate");
    const uint32_t lds_fill = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds + MXS_RING * SLOT + 3u * SLOTS_ALL * 4u + (TH / 64u) * (RT * 48u * 4u) + wave * 256u;
    // this wave's row staging area: RT x (64 lanes x 16 B), behind the fillers' scratch (the waves of different column groups
    // that work on the same rows share one)
    const uint32_t stage_off = MXS_RING * SLOT + 3u * SLOTS_ALL * 4u + (TH / 64u) * (RT * 48u * 4u) + (TH / 64u) * 256u + wig * (RT * 1024u);
    const uint32_t lds_stage = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds + stage_off;
    const uint32_t voff4 = lane * 4u;
    auto filler_ops = [&]() {
        if (KGWAS_MXS_ABLATE & 16) return;
#pragma unroll
        for (int i = 0; i < RT; i++)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(lds_fill), "v"(voff4), "s"(slab_src) : "memory");
    };
#if KGWAS_MXS_PROF
    unsigned long long pf_sync = 0, pf_step = 0, pf_epi = 0, pf_nstep = 0, pf_bar = 0, pf_issue = 0;
    const unsigned long long pf_k0 = __builtin_readcyclecounter();
#endif
    // top of step s: this wave's part of slab s + 1 has landed; B_s (every wave's part has, and every wave is through step
    // s - 1's operand reads); slab s + MXS_AHEAD goes into the slot step s - 1 read. Past the block's last step the stream simply
    // wraps around: fetched, never read, waited for before the kernel ends.
    auto step_sync = [&]() {
#if KGWAS_MXS_PROF
        const unsigned long long t0 = __builtin_readcyclecounter();
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_N) : "memory");
        const unsigned long long t1 = __builtin_readcyclecounter();
        if (!(KGWAS_MXS_ABLATE & 64)) asm volatile("s_barrier" ::: "memory");
        pf_bar += __builtin_readcyclecounter() - t1;
        pf_sync += __builtin_readcyclecounter() - t0;
#else
        if (KGWAS_MXS_ABLATE & 64)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_N) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(WAIT_N) : "memory");
#endif
    };

    filter_col_consts(a, lg * SLOTS_ALL, SLOTS_ALL, colc);
#pragma unroll
    for (uint32_t i = 0; i < MXS_AHEAD; i++) issue_slab();  // slabs 0 .. MXS_AHEAD - 1
    __syncthreads();  // (colc; the compiler's own barrier with its waits)
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");  // the first slabs are in the ring

    const uint64_t wave_row0 = blk_row0 + wig * (RT * 16u);
    auto set_rows = [&](uint32_t (&o)[RT], uint64_t rb0) {
        if (KGWAS_MXS_ABLATE & 128) rb0 &= 4095u;  // (experiments: every row load hits the L2; a wave's rows never straddle 4096)
        filter_set_rows(a, o, rb0, m);
    };
    // This lane's 16 bytes of full group g of each of its RT rows (the four kb-lanes of a row fetch the group's 64 bytes as one
    // contiguous piece; a full group's bytes always exist in the row: n_full = S / 512), requested as LDS-DMA into the wave's
    // staging area - lane l's bytes land at 16 l - and picked up with one ds_read_b128 per row tile three steps later. Through
    // LDS and not into registers: every vector-memory operation of the main loop is then one the compiler neither sees nor
    // waits for (a compiler-visible load made it drain the whole queue - slabs in flight included - where it first used the
    // data), and no register is the target of a load the compiler does not know about.
    auto request_group = [&](const uint32_t (&o)[RT], uint32_t g) {
        const uint32_t b0 = 64u * g + 16u * kb;
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            uint32_t off = o[rt] + b0;
            if (KGWAS_MXS_ABLATE & 8) off = lane * 16u;
            const uint32_t m0v = lds_stage + rt * 1024u;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(off), "s"(rows_base) : "memory");
        }
    };
    auto pickup_group = [&](uint32_t (&pc)[RT][4]) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            const uint4 v = *reinterpret_cast<const uint4*>(lds + stage_off + rt * 1024u + lane * 16u);
            pc[rt][0] = v.x;
            pc[rt][1] = v.y;
            pc[rt][2] = v.z;
            pc[rt][3] = v.w;
        }
    };
    // Slice operands of the column tiles, read from the ring one unit ahead of their MFMAs (MxOperands).
    constexpr int NU = Ops::NU;
    static_assert(NU >= 2, "at least three column tiles per wave");
    Ops B;
    B.clear();
    // operand addresses of the step whose slab lies in ring slot `slot`
    auto step_addr = [&](uint32_t slot) { return Ops::step_addr(slot * SLOT + grp * (CT * MXS_SB), lane); };
    auto read_unit = [&](int u, const MxStepAddr& sa) { B.template read_unit<0>(u, sa, lds, lane); };
    uint32_t slot_cur = 0;  // ring slot of the step about to run
    // Row pieces: `piece` = this lane's 16 bytes of the CURRENT 512-sample group of each of its RT rows. The group after it (the
    // next group of the pass or group 0 of the wave's next rows) is requested in step 1 of the current group and picked up at
    // the top of its own step 0, behind that step's wait.
    uint32_t piece[RT][4];
    uint32_t pf_ps = 0, pf_g = 0;  // the pass and group the next request fetches
    auto prefetch = [&]() {
        uint32_t o[RT];
        set_rows(o, wave_row0 + (uint64_t)pf_ps * rows_per_pass);
        request_group(o, pf_g);
        pf_g = pf_g + 1u == a.n_full ? 0u : pf_g + 1u;
        pf_ps = pf_g == 0u ? pf_ps + 1u : pf_ps;
    };
    if (a.n_full) prefetch();  // (the first group: picked up at the top of the first step, as every group's pieces are)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the steps' waits count from an empty queue)
    MxStepAddr sadr = step_addr(0);
    read_unit(0, sadr);  // step 0 of the first pass; every step's last unit fetches the next step's first
    for (uint32_t ps = 0; ps < n_passes; ps++) {
        const uint64_t rbase = wave_row0 + (uint64_t)ps * rows_per_pass;
        mxv4f acc[RT][CT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int t = 0; t < CT; t++) acc[rt][t] = (mxv4f){0.0f, 0.0f, 0.0f, 0.0f};

        // step = [B_s, slab s + AHEAD, row operations | operands A | reads of unit 1 | MFMAs of unit 0 | reads of unit 2 | MFMAs of unit 1
        //         | ... | reads of the next step's unit 0 | MFMAs of the last unit]
        // kind: 0..3 = step j of a 512-sample group (table bits from `piece`), 4 = a quarter step (operands handed in)
        auto run_step = [&](auto kind, mxv8i (&A)[RT], int sa) __attribute__((always_inline)) {
            constexpr int J = decltype(kind)::value;
            __builtin_amdgcn_sched_barrier(0);
#if KGWAS_MXS_PROF
            const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
            step_sync();
            auto vmem_ops = [&]() {  // this step's vector-memory operations: the slab MXS_AHEAD steps ahead, then RT row requests or fillers
#if KGWAS_MXS_PROF
                const unsigned long long t2 = __builtin_readcyclecounter();
#endif
                issue_slab();
                // (two column groups share rows and staging areas and BOTH request them - identical transfers, the second one an L2
                // hit. Letting only the lower group request - the upper one finds the rows behind the barrier - measured 4 % slower
                // with the same HBM-side traffic; non-temporal requests 10 % slower with 3.7 x the algorithmic traffic.)
                if (J == 1)
                    prefetch();
                else
                    filler_ops();
#if KGWAS_MXS_PROF
                pf_issue += __builtin_readcyclecounter() - t2;
#endif
            };
            vmem_ops();
            __builtin_amdgcn_sched_barrier(0);
            if (J == 0) pickup_group(piece);
            if (J < 4) mx_expand_step<0>(A, piece, J);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t slot_next = slot_cur + 1u == MXS_RING ? 0u : slot_cur + 1u;
            const MxStepAddr nadr = step_addr(slot_next);
#pragma unroll
            for (int u = 0; u < NU; u++) {
                if (u + 1 < NU)
                    read_unit(u + 1, sadr);
                else
                    read_unit(0, nadr);
                __builtin_amdgcn_sched_barrier(0);
                B.mfma_unit(u, A, acc, sa, sc0);
                __builtin_amdgcn_sched_barrier(0);
            }
            sadr = nadr;
            slot_cur = slot_next;
#if KGWAS_MXS_PROF
            pf_step += __builtin_readcyclecounter() - ts0;
            pf_nstep++;
#endif
        };

        __builtin_amdgcn_s_setprio(0);
        for (uint32_t g = 0; g < a.n_full; g++) {
            mxv8i A[RT];
            run_step(std::integral_constant<int, 0>(), A, mx_step_scale(0));
            run_step(std::integral_constant<int, 1>(), A, mx_step_scale(1));
            run_step(std::integral_constant<int, 2>(), A, mx_step_scale(2));
            run_step(std::integral_constant<int, 3>(), A, mx_step_scale(3));
        }
        // quarter groups: 128 samples per step, the lane's own dword shifted by 0..3
        uint32_t ro[RT];  // (made here, not kept across the groups' steps: eight registers the main loop has no room for)
        if (a.n_quarter) set_rows(ro, rbase);
        for (uint32_t x = 0; x < a.n_quarter; x++) {
            uint32_t b0 = 64u * a.n_full + 16u * x + 4u * kb;
            b0 = b0 + 4u <= avail_b ? b0 : avail_b - 4u;
            mxv8i A[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
                A[rt] = mx_expand_quarter((KGWAS_MXS_ABLATE & 8) ? ro[rt] + b0 : *reinterpret_cast<const uint32_t*>(rows_base + (ro[rt] + b0)));
            run_step(std::integral_constant<int, 4>(), A, mx_step_scale(0));
        }

#if KGWAS_MXS_PROF
        const unsigned long long te0 = __builtin_readcyclecounter();
#endif
        __builtin_amdgcn_s_setprio(3);  // the epilogue at raised priority (mx_kernel)
        const uint32_t tested = mx_epilogue<KGWAS_MXS_ABLATE & 1>(a, acc, wscr, colc + grp * SLOTS, colp, rbase, lane);
        if (lg == 0 && grp == 0) tested_local += tested;
#if KGWAS_MXS_PROF
        pf_epi += __builtin_readcyclecounter() - te0;
#endif
    }
#if KGWAS_MXS_PROF
    if (threadIdx.x == 0) {
        atomicAdd(&mxs_prof[0], pf_sync);
        atomicAdd(&mxs_prof[1], pf_step);
        atomicAdd(&mxs_prof[2], pf_epi);
        atomicAdd(&mxs_prof[3], pf_nstep);
        atomicAdd(&mxs_prof[4], (unsigned long long)n_passes);
        atomicAdd(&mxs_prof[5], __builtin_readcyclecounter() - pf_k0);
        atomicAdd(&mxs_prof[6], pf_bar);
        atomicAdd(&mxs_prof[7], pf_issue);
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stream's last transfers (never read) must not outlive the block's LDS
    filter_add_tested(a.tested, tested_local, lane);
}

// ring + per-column constants + the waves' row-term exchange areas + the fillers' scratch + the row staging areas
static size_t mxs_lds_bytes_t(uint32_t cta, uint32_t rt, uint32_t ng, uint32_t th, uint32_t ring) {
    const uint32_t waves = th / 64u;
    return (size_t)ring * ((cta * MXS_SB + 1023u) / 1024u * 1024u) + 3u * cta * 16u * 4u + waves * (rt * 192u) + waves * 256u + waves / ng * (rt * 1024u);
}

template <int CT, int RT, int NG, int TH>
static hipError_t launch_mxs_t(const MxArgs& a, uint32_t rows_per_block, hipStream_t st) {
    const uint32_t rpp = (TH / 64 / NG) * RT * 16u;
    // four ring slots (slabs and row requests three steps ahead) where they fit the 160 KB, else three
    const bool ring4 = mxs_lds_bytes_t(CT * NG, RT, NG, TH, 4) <= 160u * 1024u;
    const size_t lds = mxs_lds_bytes_t(CT * NG, RT, NG, TH, ring4 ? 4 : 3);
    const auto kernel = ring4 ? mxs_kernel<CT, RT, NG, TH, 4> : mxs_kernel<CT, RT, NG, TH, 3>;
    FilterGrid g;
    const hipError_t e = filter_grid((const void*)kernel, a, rpp, rows_per_block, a.n_lgroups > 1, lds, g);
    if (e != hipSuccess) return e;
    launch_last(kernel, dim3(g.grid), dim3(TH), lds, st, a, g.rows_per_block, g.n_rowblocks);
    return hipGetLastError();
}

// The streaming form exists for two slices, FP6 + FP4 (the default operand set). Shapes: CT column tiles per column group,
// NG column groups per block (a.Bq: [n_lgroups][step][NG][CT][2560 B]; a.cols: [n_lgroups][NG][CT * 16]):
//   NG = 1, CT = 3..7    eight waves, each 64 rows x CT tiles
//   NG = 2, CT = 4..7    two groups of four waves; the waves w and w + 4 work on the same 64 rows, CT tiles each (8..14 in all)
//   NG = 1, CT = 8..13   form 1: eight waves, each 32 rows x CT tiles; form 2: four waves (one per SIMD), each 64 rows x CT tiles
bool mxs_supported(uint32_t CT, uint32_t NG, uint32_t n_slices, uint32_t s1_fp6) {
    return n_slices == 2 && !s1_fp6 && ((NG == 1 && CT >= 3 && CT <= 13) || (NG == 2 && CT >= 4 && CT <= 7));
}
size_t mxs_lds_bytes(uint32_t CT, uint32_t NG) {
    const uint32_t rt = (NG == 1 && CT > 7) ? 2u : 4u;
    const size_t b4 = mxs_lds_bytes_t(CT * NG, rt, NG, 512, 4);
    return b4 <= 160u * 1024u ? b4 : mxs_lds_bytes_t(CT * NG, rt, NG, 512, 3);
}

hipError_t launch_mxs(const MxArgs& a, uint32_t CT, uint32_t NG, uint32_t form, uint32_t rows_per_block, hipStream_t st) {
    if (a.n_rows == 0) return hipSuccess;
    if (!mxs_supported(CT, NG, a.n_slices, a.s1_fp6)) return hipErrorInvalidValue;
#ifdef KGWAS_MXS_BENCH_ONLY  // experiments: the shapes of the 2048 x 201 and 1135 x 101 benches only (fast compiles)
    if (NG == 2 && CT == 7) return launch_mxs_t<7, 4, 2, 512>(a, rows_per_block, st);
    if (NG == 1 && CT == 13) return form == 2 ? launch_mxs_t<13, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<13, 2, 1, 512>(a, rows_per_block, st);
    if (NG == 1 && CT == 7) return launch_mxs_t<7, 4, 1, 512>(a, rows_per_block, st);
    return hipErrorInvalidValue;
#else
    if (NG == 2) switch (CT) {
            case 4: return launch_mxs_t<4, 4, 2, 512>(a, rows_per_block, st);
            case 5: return launch_mxs_t<5, 4, 2, 512>(a, rows_per_block, st);
            case 6: return launch_mxs_t<6, 4, 2, 512>(a, rows_per_block, st);
            case 7: return launch_mxs_t<7, 4, 2, 512>(a, rows_per_block, st);
        }
    else switch (CT) {
            case 3: return launch_mxs_t<3, 4, 1, 512>(a, rows_per_block, st);
            case 4: return launch_mxs_t<4, 4, 1, 512>(a, rows_per_block, st);
            case 5: return launch_mxs_t<5, 4, 1, 512>(a, rows_per_block, st);
            case 6: return launch_mxs_t<6, 4, 1, 512>(a, rows_per_block, st);
            case 7: return launch_mxs_t<7, 4, 1, 512>(a, rows_per_block, st);
            case 8: return form == 2 ? launch_mxs_t<8, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<8, 2, 1, 512>(a, rows_per_block, st);
            case 9: return form == 2 ? launch_mxs_t<9, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<9, 2, 1, 512>(a, rows_per_block, st);
            case 10: return form == 2 ? launch_mxs_t<10, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<10, 2, 1, 512>(a, rows_per_block, st);
            case 11: return form == 2 ? launch_mxs_t<11, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<11, 2, 1, 512>(a, rows_per_block, st);
            case 12: return form == 2 ? launch_mxs_t<12, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<12, 2, 1, 512>(a, rows_per_block, st);
            case 13: return form == 2 ? launch_mxs_t<13, 4, 1, 256>(a, rows_per_block, st) : launch_mxs_t<13, 2, 1, 512>(a, rows_per_block, st);
        }
    return hipErrorInvalidValue;
#endif
}

}  // namespace kgwas
