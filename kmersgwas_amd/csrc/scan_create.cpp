// scan_create.cpp — kgwas_scan_create: validation, then the session's plan and operands (scan_plan.cpp) on the device, its
// streams, buffers and slots, heaps and replay pool.
#include "scan_internal.h"
#include <chrono>

struct CreateTrace {  // KGWAS_TRACE: the steps of a creation on stderr
    const bool on = opt_set("KGWAS_TRACE");
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) const {
        if (on)
            fprintf(stderr, "[kgwas] scan_create +%.1f ms: %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what);
    }
};

// The parameters checked and copied into a new session; sh: its shape
static std::unique_ptr<kgwas_scan> new_session(const kgwas_scan_params* p, ScanShape& sh) {
    if (p->struct_size != sizeof(kgwas_scan_params)) throw Error(KGWAS_ERR_ARG, "kgwas_scan_params: size mismatch");
    if (!p->col || !p->Y || !p->topn || p->n_acc == 0 || p->n_pheno == 0 || p->n_acc_file == 0)
        throw Error(KGWAS_ERR_ARG, "kgwas_scan_create: empty problem");
    if (p->n_acc > p->n_acc_file) throw Error(KGWAS_ERR_ARG, "more phenotyped accessions than table columns");
    if (p->n_acc_file >= (1ull << 31)) throw Error(KGWAS_ERR_ARG, "too many accessions");
    require_heap_emulation();  // tie order = libstdc++'s heap moves (src/kmer_general.h:113-128): verified against THIS process's library
    check_device(p->device);
    KGWAS_HIP(hipSetDevice(p->device));
    std::unique_ptr<kgwas_scan> s(new kgwas_scan);
    s->device = p->device;
    s->S_f = p->n_acc_file;
    s->S = p->n_acc;
    s->W_f = (s->S_f + 63) / 64;
    s->W_m = 2 * ((s->S + 127) / 128);  // src/kmers_multiple_databases.cpp:51
    s->L = 64 * s->W_m;
    s->n_pheno = p->n_pheno;
    s->min_count = p->min_count;
    s->col.assign(p->col, p->col + s->S);
    s->topn.assign(p->topn, p->topn + s->n_pheno);
    s->Y.assign(p->Y, p->Y + s->n_pheno * s->S);
    if (p->record_history > 2) throw Error(KGWAS_ERR_ARG, "record_history: 0 (off), 1 (full log) or 2 (eviction ring)");
    s->record_history = p->record_history == 1;
    if (p->record_history == 2) {
        s->history_ring = 1;  // per heap: 16 standard deviations of the rank distance between two shards' N-th scores
        if (const char* e = opt_str("KGWAS_HISTORY_RING"))
            if (atoll(e) > 0) s->history_ring = (size_t)atoll(e);
    }
    s->count_patterns = p->count_patterns != 0;
    std::vector<bool> seen(s->S_f, false);
    for (uint64_t i = 0; i < s->S; i++) {
        if (s->col[i] >= s->S_f) throw Error(KGWAS_ERR_ARG, "column index out of range");
        if (seen[s->col[i]]) throw Error(KGWAS_ERR_ARG, "duplicate column index");
        seen[s->col[i]] = true;
    }
    for (uint64_t j = 0; j < s->n_pheno; j++) {
        if (s->topn[j] == 0) throw Error(KGWAS_ERR_ARG, "heap size must be >= 1");
        s->max_topn = std::max(s->max_topn, s->topn[j]);
        s->sum_topn += s->topn[j];
    }
    s->direct = true;
    for (uint64_t i = 0; i < s->S; i++) s->direct = s->direct && (s->col[i] == i);
    if (!s->direct) check_squeeze_fits("kgwas_scan_create", s->S_f, s->S);  // (a subset or reordered panel is squeezed per chunk)

    bool finite = true;
    for (float v : s->Y) finite = finite && std::isfinite(v);
    // The filters bound |reference yigi - exact sum| by float32 ROUNDING errors only: that needs every partial sum of
    // the reference's four chains (and their final adds) to stay finite. sum |y_i| of a column, with the growth factor
    // of recursive float32 summation, bounds them all; a column beyond that (|y| ~ 1e36 and up) can overflow to +-inf
    // in the reference on rows whose exact sum is finite - such sessions keep the exact scorers, which reproduce the
    // overflow (tests/test_gpu_parity.py::test_numeric_edges_of_the_phenotype_values[huge]).
    bool chain_safe = finite;
    for (uint64_t j = 0; j < s->n_pheno && chain_safe; j++) {
        double a = 0;
        for (uint64_t i = 0; i < s->S; i++) a += std::fabs((double)s->Y[j * s->S + i]);
        chain_safe = a * (1.0 + (double)(s->S + 8) * 0x1p-23) < 0.99 * (double)std::numeric_limits<float>::max();
    }
    sh = ScanShape{s->S, s->L, s->W_m, s->W_f, s->n_pheno, s->max_topn, s->direct, finite, chain_safe};
    return s;
}

static void create_streams(kgwas_scan* s, const CreateTrace& tcreate) {
    s->stream.create(hipStreamNonBlocking);
    tcreate("stream created (HIP context up)");
    // (Round 4 tried a side thread here that loaded the library's code objects and exercised the stream's first launch, copy
    // and cross-stream wait while this thread went on: ~20 ms of a fresh process. A fuzz run then hung INSIDE this function -
    // one helper thread spinning, this thread blocked - about once per 3 500 s of randomised sessions, never before that
    // thread existed: two threads driving the HIP runtime's allocation / registration / synchronisation paths at once is
    // not worth 20 ms. The first uses are paid where they occur.)
    s->ev_user.create();
    s->ev_ds.create();
    s->ev_dcopy.create(hipEventDisableTiming);
    s->ev_d0.create();
    s->ev_d1.create();
    tcreate("events created");
}

// The exact scorers' phenotype layouts and the small buffers on the device; returns the columns' float32 sums
static std::vector<float> upload_exact_layouts(kgwas_scan* s, const ScanShape& sh, const CreateTrace& tcreate) {
    ExactLayouts ex = exact_layouts(sh, s->col, s->Y);
    s->nb_full = ex.nb_full;
    tcreate("phenotype layouts built (host)");
    const uint64_t P = s->n_pheno;
    s->d_dmask.alloc(ex.dmask.size());
    s->d_colmap.alloc(ex.colmap.size());
    s->d_sums.alloc(P);
    s->d_thr.alloc(P);
    s->h_thr.alloc(8 * P);
    s->d_thr_host.alloc(P);
    s->d_thr_redo.alloc(P);
    s->h_thr_redo.alloc(P);
    s->d_hist.alloc(P * (size_t)HIST_BINS);
    s->d_hist_base.alloc(P);
    s->h_hist_base.alloc(P);
    s->d_pat_cnt.alloc(1);
    KGWAS_HIP(hipMemset(s->d_pat_cnt.p, 0, 8));
    KGWAS_HIP(hipMemset(s->d_thr.p, 0, P * sizeof(double)));  // 0 = "nothing is filtered" until the heaps say otherwise
    KGWAS_HIP(hipMemset(s->d_thr_host.p, 0, P * sizeof(double)));
    KGWAS_HIP(hipStreamSynchronize(nullptr));  // (null-stream memsets: the session's non-blocking streams do not wait for them)
    s->d_topn.alloc(P);
    s->d_sel.alloc(P);
    s->h_sel.alloc(P);
    s->d_sel_info.alloc(2);
    s->h_sel_info.alloc(2);
    KGWAS_HIP(hipMemcpy(s->d_topn.p, s->topn.data(), P * 8, hipMemcpyHostToDevice));
    KGWAS_HIP(hipMemcpy(s->d_dmask.p, ex.dmask.data(), ex.dmask.size() * 4, hipMemcpyHostToDevice));
    KGWAS_HIP(hipMemcpy(s->d_colmap.p, ex.colmap.data(), ex.colmap.size() * 4, hipMemcpyHostToDevice));
    KGWAS_HIP(hipMemcpy(s->d_sums.p, ex.sums.data(), P * 4, hipMemcpyHostToDevice));
    if (s->kernel_used == KGWAS_KERNEL_MFMA) {
        s->d_Ymfma.alloc(ex.Ymfma.size());
        KGWAS_HIP(hipMemcpy(s->d_Ymfma.p, ex.Ymfma.data(), ex.Ymfma.size() * 4, hipMemcpyHostToDevice));
    }
    if (s->kernel_used != KGWAS_KERNEL_MFMA || s->coarse) {
        s->d_Yperm.alloc(ex.Yperm.size());
        KGWAS_HIP(hipMemcpy(s->d_Yperm.p, ex.Yperm.data(), ex.Yperm.size() * 4, hipMemcpyHostToDevice));
    }
    tcreate("small device buffers allocated and uploaded");
    return std::move(ex.sums);
}

// The narrow filter's operands, or the planner's operand sets (fset), built on the host and uploaded
static void upload_filters(kgwas_scan* s, const ScanPlan& pl, const ScanShape& sh, const std::vector<float>& sums) {
    if (pl.narrow) {
        const NarrowOperands op = narrow_operands(sh, pl, s->Y, sums, s->dbg_keep_resid ? s->dbg_resid[2].data() : nullptr);
        s->d_Bn.alloc(op.Bn.size());
        s->d_ncols.alloc(sh.P);
        KGWAS_HIP(hipMemcpy(s->d_Bn.p, op.Bn.data(), op.Bn.size(), hipMemcpyHostToDevice));
        KGWAS_HIP(hipMemcpy(s->d_ncols.p, op.ncols.data(), sh.P * sizeof(NarrowCol), hipMemcpyHostToDevice));
    }
    for (int mi = 0; mi < 2; mi++) {
        if (!pl.set[mi].slices) continue;
        kgwas_scan::DeviceFilterSet& M = s->fset[mi];
        M.plan = pl.set[mi];
        const FilterSet& fs = M.plan;
        if (fs.mx) M.scale0 = 0x01010101u * (uint32_t)(0x7F + (fs.slices == 1 ? 0 : 5));
        uint32_t groups_all = 0;
        for (size_t pi = 0; pi < fs.parts.size(); pi++) {
            const FilterPart& fp = fs.parts[pi];
            if (fp.stream) s->st.coarse_mx_stream = fp.stream;
            groups_all += fp.launch_groups();
            double* resid = s->dbg_keep_resid ? s->dbg_resid[mi].data() : nullptr;
            const PartOperands op = fs.mx ? block_scaled_operands(sh, fs, fp, s->Y, sums, resid)
                                          : int8_operands(sh, pl.n_kgroups, fs, fp, s->Y, sums, resid);
            M.eg_max = std::max(M.eg_max, op.eg_max);
            M.rall_max = std::max(M.rall_max, op.rall_max);
            M.rmax_max = std::max(M.rmax_max, op.rmax_max);
            M.dev[pi].d_Bq.alloc(op.Bq.size());
            M.dev[pi].d_cols.alloc(op.cols.size());
            KGWAS_HIP(hipMemcpy(M.dev[pi].d_Bq.p, op.Bq.data(), op.Bq.size(), hipMemcpyHostToDevice));
            KGWAS_HIP(hipMemcpy(M.dev[pi].d_cols.p, op.cols.data(), op.cols.size() * sizeof(CoarseCol), hipMemcpyHostToDevice));
        }
        s->st.coarse_mode_tiles[mi] = fs.parts.empty() ? 0 : fs.parts[0].T;
        s->st.coarse_mode_lgroups[mi] = groups_all;
        s->st.coarse_mode_tile_slices[mi] = fs.tile_slices;
        if (fs.mx) {
            if (pl.use_mx) s->st.coarse_mx = 1;
            s->st.coarse_mx_s1_fp6 = fs.s1_fp6;
            s->st.coarse_mx_steps = fs.n_steps;
        }
        M.ready = true;
    }
}

// The filter's survivor keys, bitmap and re-score buffers, and the copy stream of its records
static void alloc_filter_buffers(kgwas_scan* s) {
    const uint64_t P = s->n_pheno;
    s->key_slots = (uint32_t)std::min<uint64_t>((uint64_t)s->cap * P, 0x7FFFFFFFull);
    s->d_surv_sorted.alloc(s->key_slots);
    s->bitmap_words = (s->chunk_max + 63) / 64;
    s->d_bitmap.alloc(P * s->bitmap_words);
    s->d_bm_blocks.alloc(P * ((s->bitmap_words + 1023) / 1024 + 1) + 4);
    if (!s->narrow) s->d_bm_mask.alloc(P * ((s->bitmap_words + 1023) / 1024) * 4 + 4);
    s->bitmap_clean = false;
    s->d_surv_cnt.alloc(P);
    s->d_surv_off.alloc(P);
    s->d_key_count.alloc(1);  // the survivor count
    s->d_tile_pref.alloc(P + 1);
    s->d_tile_cnt.alloc((size_t)s->key_slots / 256 + P + 2);
    s->d_tmp_score.alloc(s->key_slots);
    // The record copies run as blit kernels (rocprofv3 shows __amd_rocclr_copyBuffer, not SDMA transfers), and at
    // normal priority they are only dispatched in the gaps of the compute stream: behind a 0.75 ms filter launch
    // of a one-column scan, a chunk's 1 MB of records reached the host 1.3-2.8 ms after its counts. A high-priority
    // queue gets them onto the chip between the running launch's workgroups. KGWAS_COPY_PRIO=0: the old behaviour.
    int least = 0, greatest = 0;
    KGWAS_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const bool hi = !(exp_int("KGWAS_COPY_PRIO", 1) == 0);
    s->copy_stream.create_with_priority(hipStreamNonBlocking, hi ? greatest : least);
    s->row_key_bits = 1;
    while (s->row_key_bits < 32 && (1ull << s->row_key_bits) < s->chunk_max) s->row_key_bits++;
}

// The squeeze buffer, the slots of chunks in flight (and the pinned record ring they fill) and the dense-mode buffers
static void alloc_slots(kgwas_scan* s, const CreateTrace& tcreate) {
    const uint64_t P = s->n_pheno;
    if (!s->direct) s->d_sq.alloc(s->chunk_max * 2 * s->W_m);
    if (s->coarse) {
        // device side: 20 B x key_slots of HBM per slot, up to 4 GiB in all; host side: the record ring
        const uint64_t slot_bytes = (uint64_t)s->key_slots * 20;
        s->n_slots = (int)std::min<uint64_t>(MAX_SLOTS, std::max<uint64_t>(4, (4ull << 30) / std::max<uint64_t>(slot_bytes, 1)));
        const char* forced = opt_str("KGWAS_RING_BYTES");  // (tests)
        s->rr.set_size(record_ring_bytes((uint64_t)s->n_slots, slot_bytes, forced ? std::max<uint64_t>(strtoull(forced, nullptr, 10), 1) : 0));
        tcreate("device buffers and slots allocated");
        s->ring.alloc(s->rr.size());
        s->ring_dev = s->ring.dev();
        tcreate("pinned record ring allocated");
    } else {
        const uint64_t slot_bytes = (uint64_t)s->cap * P * sizeof(Cand);
        s->n_slots = (int)std::min<uint64_t>(16, std::max<uint64_t>(4, (1ull << 30) / std::max<uint64_t>(slot_bytes, 1)));
    }
    for (int si = 0; si < s->n_slots + (s->coarse ? 1 : 0); si++) {
        const bool is_redo = si == s->n_slots;
        Slot& sl = is_redo ? s->redo : s->slot[si];
        if (s->coarse && !is_redo) {
            sl.d_so_score.alloc(s->key_slots);
            sl.d_so_kmer.alloc(s->key_slots);
            sl.d_so_row.alloc(s->key_slots);
            sl.d_meta.alloc(2 * P + 4);
            sl.h_meta.alloc(2 * P + 4);
            sl.h_thr.alloc(P);
            memset(sl.h_thr.p, 0, P * sizeof(double));
            memset(sl.h_meta.p, 0, (2 * P + 4) * sizeof(uint32_t));
            sl.h_meta_dev = sl.h_meta.dev();
            sl.h_thr_dev = sl.h_thr.dev();
            sl.ev_counts.create(hipEventBlockingSync);
        } else {
            sl.cand.alloc((uint64_t)s->cap * P);
            sl.d_cand = sl.cand.dev();
        }
        sl.d_cnt.alloc(P);
        sl.h_cnt.alloc(P);
        sl.d_tested.alloc(TESTED_SHARDS);
        sl.h_tested.alloc(TESTED_SHARDS);
        sl.h_tested_dev = sl.h_tested.dev();
        sl.ev_sq0.create();
        sl.ev_k0.create();
        sl.ev_k1.create();
        // (blocking wait: the control thread sleeps instead of spinning beside the replay workers)
        sl.ev_done.create(hipEventBlockingSync);
        sl.ev_mid.create();
    }
    s->d_dense.alloc(P * s->dense_rows);
    s->h_dense.alloc(P * s->dense_rows);
    s->d_n1.alloc(s->dense_rows);
    s->h_n1.alloc(s->dense_rows);
    s->d_kmer.alloc(s->dense_rows);
    s->h_kmer.alloc(s->dense_rows);
    s->h_dense_dev = s->h_dense.dev();
    s->h_n1_dev = s->h_n1.dev();
    s->h_kmer_dev = s->h_kmer.dev();
    s->d_tested_dense.alloc(TESTED_SHARDS);
}

// The heaps, and the columns that select their top N instead of replaying it (scan_lazy.cpp)
static void make_heaps_and_select(kgwas_scan* s) {
    make_heaps(s);
    const char* fr = opt_str("KGWAS_FULL_REPLAY");
    s->lazy_enabled = s->coarse && !s->record_history && !(fr && atoi(fr) != 0);
    s->lazy_log_mode = s->lazy_enabled && s->history_ring != 0;
    lazy_reset(s);
    s->hist.resize(s->n_pheno);
    s->keys.resize(s->n_pheno);
    s->col_ms.assign(s->n_pheno, 0.0);
}

// The replay threads and the column groups they take
static void make_replay_pool(kgwas_scan* s, const kgwas_scan_params& p) {
    const uint64_t P = s->n_pheno;
    s->trace = opt_set("KGWAS_TRACE");
    unsigned nt = p.host_threads ? p.host_threads : usable_cpus();
    if (const char* e = opt_str("KGWAS_HOST_THREADS"))
        if (atoi(e) > 0) nt = (unsigned)atoi(e);
    nt = (unsigned)std::min<uint64_t>(nt, P);
    s->pool.reset(new Pool(nt, pick_replay_cpus(nt, s->device)));
    s->st.replay_threads = nt;
    s->ingest.producer_cpus_ = p.host_threads ? p.host_threads : usable_cpus();
    // Column groups of the replay. Worker w owns the columns w, w + T, ... of the first floor(P / T) * T columns,
    // in groups of at most MAX_LOCKSTEP (a group's heaps take their replacements in lockstep, and stay in their
    // worker's cache from chunk to chunk); the P mod T columns left over float: each is a group of its own that
    // whichever worker is furthest ahead takes, which evens out what a static map cannot (101 columns on 16
    // workers is 5 x 7 + 11 x 6: the 7-column workers set the pace, 17 % above the mean).
    const uint64_t T = nt, base = P / T;
    const uint64_t MKc = (uint64_t)BestHeap::MAX_LOCKSTEP;
    uint64_t per = base ? (base + ((base + MKc - 1) / MKc) - 1) / ((base + MKc - 1) / MKc) : 0;  // balanced split
    if (const char* e = exp_str("KGWAS_REPLAY_GROUP"))
        if (atoi(e) > 0 && per) per = std::min<uint64_t>((uint64_t)atoi(e), MKc);
    for (uint64_t w = 0; w < T && base; w++) {
        std::vector<uint32_t> cur;
        for (uint64_t i = 0; i < base; i++) {
            cur.push_back((uint32_t)(i * T + w));
            if (cur.size() == per || i + 1 == base) {
                s->grp_cols.push_back(cur);
                s->grp_home.push_back((int)w);
                cur.clear();
            }
        }
    }
    for (uint64_t j = base * T; j < P; j++) {
        s->grp_cols.push_back(std::vector<uint32_t>(1, (uint32_t)j));
        s->grp_home.push_back(-1);
    }
    s->n_groups0 = s->grp_cols.size();
    s->n_groups.store(s->n_groups0);
    s->grp_cols0 = s->grp_cols;
    const size_t cap = s->n_groups0 + (size_t)P;  // room for every column as a group of its own (split_group)
    s->grp_cols.resize(cap);
    s->gstate.reset(new kgwas_scan::GroupState[cap]);
    s->grp_owner.reset(new std::atomic<int>[cap]);
    s->col_popped.reset(new std::atomic<uint8_t>[(size_t)P]);
    for (uint64_t j = 0; j < P; j++) s->col_popped[j].store(0);
    s->res_kmer.resize(P);
    s->res_row.resize(P);
    s->res_score.resize(P);
    for (size_t g = 0; g < cap; g++) s->grp_owner[g].store(g < s->n_groups0 ? s->grp_home[g] : -1);
    if (const char* e = opt_str("KGWAS_SPLIT_LAGGING")) s->split_lagging = atoi(e) != 0;
    if (const char* e = opt_str("KGWAS_FLOAT_LEAD")) s->float_lead = (uint64_t)std::max(0, atoi(e));
    if (const char* e = opt_str("KGWAS_DEBUG_SLOW_WORKER")) {
        int w = -1, pct = 100, min_us = 0;
        if (sscanf(e, "%d:%d:%d", &w, &pct, &min_us) >= 1) {
            s->dbg_slow_worker = w;
            s->dbg_slow_pct = pct;
            s->dbg_slow_min_us = min_us;
        }
    }
    s->slot_left.reset(new std::atomic<uint32_t>[MAX_SLOTS]);
    for (int i = 0; i < MAX_SLOTS; i++) s->slot_left[i].store(0);
    s->rp_fn = [s](size_t w) { replay_worker(s, w); };
}

extern "C" {

int kgwas_scan_create(const kgwas_scan_params* p, kgwas_scan** out) {
    return guarded([&] {
        if (!p || !out) throw Error(KGWAS_ERR_ARG, "kgwas_scan_create: null argument");
        ScanShape sh;
        std::unique_ptr<kgwas_scan> s = new_session(p, sh);
        const FilterOpts opts = read_filter_opts();
        const ScanPlan pl = plan_scan(*p, sh, opts, s->Y, s->dbg_resid);
        s->kernel_used = pl.kernel;
        s->coarse = pl.coarse;
        s->narrow = pl.narrow;
        s->narrow_pack1 = pl.narrow_pack1;
        s->n_kgroups = pl.n_kgroups;
        s->chunk_max = pl.chunk_max;
        s->dense_rows = pl.dense_rows;
        s->dense_chunk = pl.dense_chunk;
        s->cap = pl.cap;
        s->mode_k = opts.mode_k;
        s->dbg_keep_resid = pl.keep_resid;
        s->dbg_keep_surv = pl.keep_surv;

        const CreateTrace tcreate;
        create_streams(s.get(), tcreate);
        const std::vector<float> sums = upload_exact_layouts(s.get(), sh, tcreate);
        if (s->coarse) {
            upload_filters(s.get(), pl, sh, sums);
            tcreate("operand sets built and uploaded");
            alloc_filter_buffers(s.get());
        }
        alloc_slots(s.get(), tcreate);
        make_heaps_and_select(s.get());
        tcreate("buffers done");
        make_replay_pool(s.get(), *p);
        s->st.kernel_used = s->narrow ? (uint32_t)KGWAS_KERNEL_NARROW : s->coarse ? (uint32_t)KGWAS_KERNEL_COARSE : pl.kernel;
        s->st.direct_mode = s->direct ? 1 : 0;
        tcreate("pool, heaps and arena ready");
        *out = s.release();
    });
}

}  // extern "C"
