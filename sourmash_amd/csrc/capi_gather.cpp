// capi_gather.cpp -- the C-ABI (include/sourmash_amd.h): gather over a device-resident collection (gather.hip, gather_build.hip),
// its rounds shared between ranks, and the raw overlap / set operations on caller-owned device buffers (overlap.hip, pair_ops.hip).
#include <fcntl.h>
#include <stdio.h>
#include <sys/mman.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <memory>
#include "capi_common.hpp"

using namespace smg;

namespace {

// ---- device-resident sketch collections and gather counters ------------------------------------
struct GatherCounter {
    const SketchSet* set = nullptr;
    DevBuf q, list, scal;
    uint64_t nq = 0;
    GatherDev g;
    ~GatherCounter() { gather_destroy(g); }          // (q / list / scal: arena blocks, released by their DevBufs)
};
// raw variant: query and database are caller-owned device buffers (torch tensors)
struct GatherRaw {
    GatherDev g;
    ~GatherRaw() { gather_destroy(g); }
};

// run the armed loop to exhaustion; -> number of results (host copies if out_* given).
// Two device loops with identical results: "scan" (default) picks the arg-max over all counters every round; "replay"
// runs the multi-GPU protocol with one shard (the 16 best rows exported, rounds replayed among those candidates while
// the best stays above the best key kept back).  Measured on one GPU (profiles/r02_gather_loops.txt): replay wins only
// when the leading counters are well separated; with clustered counters (config C5: every round lowers all of them by
// a few hashes, so the kept-back key overtakes after ~3 rounds) the extra exchanges make it slower, 69 vs 29 us / round.
static bool gather_use_replay() {
    static const int mode = [] {
        const char* e = getenv("SMG_GATHER_LOOP");
        return e && !strcmp(e, "replay") ? 1 : 0;
    }();
    return mode == 1;
}
// Persistent-loop exit codes that mean "gave up waiting" rather than "broken" (gather.hip: the gate 10, the sweeps 11-13, a peer
// rank's gate 14).  Only the GATE codes are a decision of the grid as a whole: one word decides, nothing has been touched, and
// the rounds can carry on in place from the same state.  11-13 are per-workgroup spin limits inside a round: workgroup X can
// leave at epoch e while workgroup Z, whose sweep began later, still sees the late record and applies round e -- the written-back
// counters and uncovered set then belong to different round counts.  After those the state is void: single-rank callers get the
// error, gather_distributed builds a fresh index and runs the record protocol (parallel.py).
static bool gather_loop_gave_up(unsigned long long code) { return code >= 10 && code <= 14; }
static bool gather_loop_state_untouched(unsigned long long code) { return code == 10 || code == 14; }
static uint64_t gather_drain(GatherDev& g, uint64_t* out_idx, uint64_t* out_isect, uint64_t cap, hipStream_t st) {
    unsigned long long head[GS_SLOTS];
    const bool replay = gather_use_replay() && g.ndb > 0 && g.nq > 0;
    static const bool trace = getenv("SMG_GATHER_TRACE") != nullptr;   // per batch: time to enqueue, time until the GPU is through
    // SMG_GATHER_GRAPH: 0 eager launches only, 1 graph replays only, unset: eager until a batch shows the host cannot keep
    // ahead (the GPU was through almost as soon as the last launch was issued), then graph replays of 64 rounds
    static const int graph_mode = [] { const char* e = getenv("SMG_GATHER_GRAPH"); return e ? atoi(e) : -1; }();
    bool use_graph = graph_mode == 1;
    unsigned batch = 32;
    const auto t_all = std::chrono::steady_clock::now();
    hipEvent_t ev0 = nullptr, ev1 = nullptr;                           // GPU span of the rounds (smgpu_gather_stats)
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev_guard{ev0, ev1};
    hip_check(hipEventCreate(&ev0), "event");
    hip_check(hipEventCreate(&ev1), "event");
    hip_check(hipEventRecord(ev0, st), "event");
    bool graph_synced = false;
    double gpu_ms_graph = 0.0;
    // the whole loop as one resident kernel when the index allows it (gather.hip: gather_loop_kernel)
    bool persistent = false;
    if (!replay && graph_mode != 1) hip_check(gather_run_persistent(g, st, &persistent), "gather loop (persistent)");
    if (persistent) {
        hip_check(hipMemcpyAsync(g.pinned + 16, g.state, sizeof(head), hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        memcpy(head, g.pinned + 16, sizeof(head));
        if (head[GS_ERR]) {
            // The grid did not become resident as a whole (another kernel or another process holds CUs): the kernel gave up at
            // its gate with nothing touched (code 10) and the two-kernel rounds below carry on from exactly that state -- a
            // library inside somebody's process cannot ask for an idle device.  Anything else -- a spin limit inside a round
            // (11-13: not a grid-wide decision, see above), a staged row that never arrived (2-4) -- is an error.
            if (!gather_loop_state_untouched(head[GS_ERR]))
                throw err_internal("gather loop failed (code " + std::to_string(head[GS_ERR]) + ", epoch " + std::to_string(head[13]) +
                                   ", workgroup " + std::to_string(head[14]) + "): the index's counters are void, build it again");
            if (trace)
                fprintf(stderr, "[gather] persistent loop gave up (code %llu, workgroup %llu) after %llu rounds, %.1f us: two-kernel rounds take over\n",
                        head[GS_ERR], head[14], head[GS_ROUNDS], std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_all).count());
            hip_check(hipMemsetAsync(g.state + GS_ERR, 0, 8, st), "memset");
            g.loop_fallbacks++;
            persistent = false;
        } else if (trace)
            fprintf(stderr, "[gather] persistent loop: %llu rounds, %.1f us\n", head[GS_ROUNDS],
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_all).count());
    }
    for (; !persistent;) {
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t bs = st;                                           // the stream this batch runs on
        if (use_graph && !graph_synced) {                              // the graph runs on the index's own stream: everything
            hip_check(hipStreamSynchronize(st), "sync");               // enqueued on the caller's stream (begin, earlier batches) first
            graph_synced = true;
        }
        if (replay) hip_check(gather_enqueue_replay(g, (batch + GATHER_TOPK_MAX - 1) / GATHER_TOPK_MAX, st), "gather rounds");
        else if (use_graph) hip_check(gather_enqueue_rounds_graph(g, batch, &bs), "gather rounds (graph)");
        else hip_check(gather_enqueue_rounds(g, batch, st), "gather rounds");
        const auto t1 = std::chrono::steady_clock::now();
        hip_check(hipMemcpyAsync(g.pinned + 16, g.state, sizeof(head), hipMemcpyDeviceToHost, bs), "D2H");
        hip_check(hipStreamSynchronize(bs), "sync");
        memcpy(head, g.pinned + 16, sizeof(head));
        if (bs != st) gpu_ms_graph += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const double enqueue_us = std::chrono::duration<double, std::micro>(t1 - t0).count();
        const double wait_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
        if (trace)
            fprintf(stderr, "[gather] batch of %u rounds (%s): enqueue %.1f us, then %.1f us until done (rounds so far %llu; %.1f us since the loop began)\n",
                    batch, replay ? "replay" : use_graph ? "graph" : "eager", enqueue_us, wait_us, head[GS_ROUNDS],
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_all).count());
        if (head[GS_DONE]) break;
        if (!replay && !use_graph && graph_mode == -1 && batch >= 64 && wait_us < 0.2 * enqueue_us) use_graph = true;
        if (batch < 512) batch *= 2;
    }
    const uint64_t n = head[GS_ROUNDS];
    const uint64_t m = n < cap ? n : cap;
    hip_check(hipEventRecord(ev1, st), "event");
    if (m && out_idx) hip_check(hipMemcpyAsync(out_idx, g.out_idx, m * 8, hipMemcpyDeviceToHost, st), "D2H");
    if (m && out_isect) hip_check(hipMemcpyAsync(out_isect, g.out_isect, m * 8, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    float span = 0.f;
    (void)hipEventElapsedTime(&span, ev0, ev1);
    g.loop_gpu_ms = span + gpu_ms_graph;                               // graph batches run on another stream: their wall clock
    g.loop_host_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_all).count();
    if (trace)
        fprintf(stderr, "[gather] %llu rounds read back; %.1f us since the loop began\n", (unsigned long long)n,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_all).count());
    return n;
}

// ---- several ranks running the same gather rounds through shared host memory (gather.hip: gather_launch_loop) ----
struct GatherXchg {
    unsigned long long* host = nullptr;      // the mapping in this process
    unsigned long long* dev = nullptr;       // its device-visible address
    size_t bytes = 0;
    uint32_t world = 0;
    uint64_t rowcap = 0;
    std::string shm_name;                    // "" : private pinned memory (one process drives every rank)
    bool creator = false, registered = false;
    // device kind: this rank's area lives in its own device memory, the peers' areas are mapped in through hipIpc handles
    bool device = false;
    uint32_t rank = 0;
    unsigned long long* own = nullptr;
    std::vector<unsigned long long*> peers;  // [world] device-visible address of every rank's area (own included)
    std::vector<void*> opened;               // mappings to close
    ~GatherXchg() {
        if (device) {
            for (void* p : opened) (void)hipIpcCloseMemHandle(p);
            if (own) (void)hipFree(own);     // (not an arena block: IPC handles are per allocation; freed once per process lifetime)
            return;
        }
        if (!host) return;
        if (shm_name.empty()) (void)hipHostFree(host);
        else {
            if (registered) (void)hipHostUnregister(host);
            munmap(host, bytes);
            if (creator) shm_unlink(shm_name.c_str());
        }
    }
};

static void select_pair(const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* d_out, uint64_t* d_n,
                        void* d_ws, uint64_t ws_bytes, int invert, void* stream) {
    landing_void([&] {
        if (ws_bytes < smgpu_intersect_workspace_bytes(na)) throw err_internal("workspace too small (smgpu_intersect_workspace_bytes)");
        uint8_t* flags = (uint8_t*)d_ws;
        void* tmp = (char*)d_ws + ((na + 255) / 256) * 256;
        const size_t tmp_bytes = (size_t)(ws_bytes - ((na + 255) / 256) * 256);
        hipStream_t st = (hipStream_t)stream;
        hip_check(pair_match_launch(d_a, na, d_b, nb, nullptr, nullptr, flags, nullptr, invert, st), "pair_match");
        hip_check(select_flagged(d_a, flags, na, d_out, d_n, tmp, tmp_bytes, st), "select");
    });
}

}  // namespace

uint64_t smg::gather_one_on_device(const uint64_t* d_query, uint64_t nq, const SketchSet& db, uint64_t threshold_hashes, std::vector<uint64_t>& idx,
                                   std::vector<uint64_t>& isect, hipStream_t st) {
    GatherRaw r;
    r.g.Q = d_query;
    r.g.nq = nq;
    r.g.hashes = db.hashes.as<uint64_t>();
    r.g.offsets = db.offsets.as<uint64_t>();
    r.g.ndb = db.n;
    r.g.index_base = 0;
    hip_check(gather_build(r.g, st), "gather index");
    hip_check(gather_begin(r.g, threshold_hashes, db.n ? db.n : 1, st), "gather arm");
    const uint64_t cap = db.n ? db.n : 1;
    idx.assign(cap, 0);
    isect.assign(cap, 0);
    const uint64_t rounds = gather_drain(r.g, idx.data(), isect.data(), cap, st);
    idx.resize((size_t)std::min(rounds, cap));
    isect.resize(idx.size());
    return rounds;
}

extern "C" {

SmgpuCounter* smgpu_counter_new(const SmgpuSketchSet* set, const SourmashKmerMinHash* query) {
    return landing<SmgpuCounter*>([&]() -> SmgpuCounter* {
        const SketchSet* s = reinterpret_cast<const SketchSet*>(set);
        (void)MH(query);                                              // queued records are hashed before the context is taken
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        std::unique_ptr<GatherCounter> c(new GatherCounter());
        c->set = s;
        c->nq = MH(query)->size();
        c->q.reserve(c->nq * 8 + 16, st);
        c->scal.reserve(64, st);
        if (c->nq) hip_check(hipMemcpyAsync(c->q.p, MH(query)->mins.data(), c->nq * 8, hipMemcpyHostToDevice, st), "H2D");
        c->g.Q = c->q.as<uint64_t>();
        c->g.nq = c->nq;
        c->g.hashes = s->hashes.as<uint64_t>();
        c->g.offsets = s->offsets.as<uint64_t>();
        c->g.ndb = s->n;
        c->g.index_base = 0;
        hip_check(gather_build(c->g, st), "gather index");        // postings + counters = |Q ∩ D_d| for every d
        hip_check(gather_begin(c->g, 0, s->n ? s->n : 1, st), "gather arm");
        return reinterpret_cast<SmgpuCounter*>(c.release());
    });
}
void smgpu_counter_free(SmgpuCounter* p) { delete reinterpret_cast<GatherCounter*>(p); }
void smgpu_counter_get(const SmgpuCounter* p, uint64_t* out) {
    landing_void([&] {
        const GatherCounter* c = reinterpret_cast<const GatherCounter*>(p);
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        if (c->set->n) hip_check(hipMemcpyAsync(out, c->g.counters, c->set->n * 8, hipMemcpyDeviceToHost, ctx.stream()), "D2H");
        hip_check(hipStreamSynchronize(ctx.stream()), "sync");
    });
}
void smgpu_counter_set(SmgpuCounter* p, uint64_t index, uint64_t value) {
    landing_void([&] {
        GatherCounter* c = reinterpret_cast<GatherCounter*>(p);
        if (index >= c->set->n) throw err_internal("counter index out of range");
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        c->g.counters_touched = true;
        hip_check(hipMemcpyAsync(c->g.counters + index, &value, 8, hipMemcpyHostToDevice, ctx.stream()), "H2D");
        hip_check(hipStreamSynchronize(ctx.stream()), "sync");
    });
}
bool smgpu_counter_best(const SmgpuCounter* p, uint64_t* index, uint64_t* count) {
    return landing<bool>([&]() -> bool {
        GatherCounter* c = const_cast<GatherCounter*>(reinterpret_cast<const GatherCounter*>(p));
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        unsigned long long* d_best = c->scal.as<unsigned long long>();
        hip_check(hipMemsetAsync(d_best, 0, 8, st), "memset");
        hip_check(argmax_launch(c->g.counters, c->set->n, 0, d_best, st), "argmax");
        unsigned long long key = 0;
        hip_check(hipMemcpyAsync(&key, d_best, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        if (key == 0) return false;
        *count = key >> 32;
        *index = gather_key_index(key);
        return true;
    });
}
void smgpu_counter_consume(SmgpuCounter* p, const SourmashKmerMinHash* intersect) {
    landing_void([&] {
        GatherCounter* c = reinterpret_cast<GatherCounter*>(p);
        const uint64_t ni = MH(intersect)->size();
        if (ni == 0) return;
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        c->list.reserve((ni + 1) * 8 + 16, st);
        uint64_t* d_list = c->list.as<uint64_t>();
        hip_check(hipMemcpyAsync(d_list, &ni, 8, hipMemcpyHostToDevice, st), "H2D");
        hip_check(hipMemcpyAsync(d_list + 1, MH(intersect)->mins.data(), ni * 8, hipMemcpyHostToDevice, st), "H2D");
        // the postings cover hashes of the original query only; an intersect holding anything else (a caller
        // outside the peek/consume protocol) takes the streaming kernel over the whole database instead
        unsigned long long* d_hits = c->scal.as<unsigned long long>() + 1;
        hip_check(hipMemsetAsync(d_hits, 0, 32, st), "memset");
        hip_check(pair_match_launch(d_list + 1, ni, c->g.Q, c->nq, nullptr, nullptr, nullptr, d_hits, 0, st), "pair_match");
        unsigned long long hits = 0;
        hip_check(hipMemcpyAsync(&hits, d_hits, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        if (hits == ni)
            hip_check(gather_consume_list(c->g, d_list, st), "consume");
        else
            hip_check(overlap_vector_launch(d_list + 1, ni, c->set->hashes.as<uint64_t>(), c->set->offsets.as<uint64_t>(),
                                            c->set->n, c->g.counters, 1, st), "consume");
        hip_check(hipStreamSynchronize(st), "sync");
    });
}
uint64_t smgpu_counter_gather(SmgpuCounter* p, uint64_t threshold_hashes, uint64_t* out_index, uint64_t* out_isect,
                              uint64_t cap) {
    return landing<uint64_t>([&]() -> uint64_t {
        GatherCounter* c = reinterpret_cast<GatherCounter*>(p);
        DeviceCtx& ctx = DeviceCtx::get();
        std::lock_guard<std::recursive_mutex> g(ctx.mutex());
        hipStream_t st = ctx.stream();
        hip_check(gather_begin(c->g, threshold_hashes, c->set->n ? c->set->n : 1, st), "gather arm");
        return gather_drain(c->g, out_index, out_isect, cap, st);
    });
}

// ---- raw gather over caller-owned device buffers ----------------------------------------------------------------
SmgpuGather* smgpu_gather_new_raw(const uint64_t* d_query, uint64_t nq, const uint64_t* d_hashes, const uint64_t* d_offsets,
                                  uint64_t ndb, uint64_t index_base, void* stream) {
    return landing<SmgpuGather*>([&]() -> SmgpuGather* {
        std::unique_ptr<GatherRaw> r(new GatherRaw());
        r->g.Q = d_query;
        r->g.nq = nq;
        r->g.hashes = d_hashes;
        r->g.offsets = d_offsets;
        r->g.ndb = ndb;
        r->g.index_base = index_base;
        hip_check(gather_build(r->g, (hipStream_t)stream), "gather index");
        return reinterpret_cast<SmgpuGather*>(r.release());
    });
}
void smgpu_gather_free(SmgpuGather* p) { delete reinterpret_cast<GatherRaw*>(p); }
uint64_t smgpu_gather_postings(const SmgpuGather* p) { return reinterpret_cast<const GatherRaw*>(p)->g.npairs; }
void smgpu_gather_stats(SmgpuGather* p, double* out) {
    landing_void([&] {
        GatherDev& g = reinterpret_cast<GatherRaw*>(p)->g;
        float ms = 0.f;
        hip_check(gather_build_kernel_ms(g, &ms), "build events");
        out[0] = ms;
        out[1] = g.build_host_ns * 1e-6;
        out[2] = g.build_driver_ns * 1e-6;
        out[3] = (double)g.build_driver_allocs;
        out[4] = (double)g.build_syncs;
        out[5] = g.build_sync_wait_ns * 1e-6;
        out[6] = g.loop_gpu_ms;
        out[7] = g.loop_host_ns * 1e-6;
        out[8] = (double)g.loop_fallbacks;
    });
}

void smgpu_gather_counters_get(const SmgpuGather* p, uint64_t* out, void* stream) {
    landing_void([&] {
        const GatherDev& g = reinterpret_cast<const GatherRaw*>(p)->g;
        if (g.ndb) hip_check(hipMemcpyAsync(out, g.counters, g.ndb * 8, hipMemcpyDeviceToHost, (hipStream_t)stream), "D2H");
        hip_check(hipStreamSynchronize((hipStream_t)stream), "sync");
    });
}
void smgpu_gather_begin(SmgpuGather* p, uint64_t threshold_hashes, uint64_t max_rounds, void* stream) {
    landing_void([&] {
        hip_check(gather_begin(reinterpret_cast<GatherRaw*>(p)->g, threshold_hashes, max_rounds, (hipStream_t)stream),
                  "gather arm");
    });
}
uint64_t smgpu_gather_run(SmgpuGather* p, uint64_t* out_index, uint64_t* out_isect, uint64_t cap, void* stream) {
    return landing<uint64_t>([&]() -> uint64_t {
        return gather_drain(reinterpret_cast<GatherRaw*>(p)->g, out_index, out_isect, cap, (hipStream_t)stream);
    });
}

SmgpuGatherXchg* smgpu_gather_xchg_new(const char* shm_name, uint32_t world, uint64_t rowcap, bool create) {
    return landing<SmgpuGatherXchg*>([&]() -> SmgpuGatherXchg* {
        if (world == 0 || world > 1024 || rowcap == 0) throw err_internal("gather exchange: bad geometry");
        std::unique_ptr<GatherXchg> x(new GatherXchg());
        x->world = world; x->rowcap = rowcap;
        x->bytes = ((size_t)2 * world * 4 + (size_t)2 * world * rowcap) * 8;
        x->bytes = (x->bytes + 4095) & ~(size_t)4095;
        if (!shm_name || !*shm_name) {
            hip_check(hipHostMalloc((void**)&x->host, x->bytes, hipHostMallocDefault), "hipHostMalloc");
            memset(x->host, 0, x->bytes);
            x->dev = x->host;
        } else {
            x->shm_name = shm_name;
            x->creator = create;
            const int fd = shm_open(shm_name, create ? (O_CREAT | O_EXCL | O_RDWR) : O_RDWR, 0600);
            if (fd < 0) throw err_internal(std::string("gather exchange: shm_open(") + shm_name + ") failed");
            if (create && ftruncate(fd, (off_t)x->bytes) != 0) { ::close(fd); shm_unlink(shm_name); throw err_internal("gather exchange: ftruncate failed"); }
            void* m = mmap(nullptr, x->bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
            ::close(fd);
            if (m == MAP_FAILED) { if (create) shm_unlink(shm_name); throw err_internal("gather exchange: mmap failed"); }
            x->host = (unsigned long long*)m;
            if (create) memset(x->host, 0, x->bytes);
            hip_check(hipHostRegister(x->host, x->bytes, hipHostRegisterPortable | hipHostRegisterMapped), "hipHostRegister");
            x->registered = true;
            void* d = nullptr;
            hip_check(hipHostGetDevicePointer(&d, x->host, 0), "hipHostGetDevicePointer");
            x->dev = (unsigned long long*)d;
        }
        return reinterpret_cast<SmgpuGatherXchg*>(x.release());
    });
}
// The exchange in DEVICE memory (north_star: "over xGMI"): every rank owns one area -- [2][4] record granules + [2][rowcap] row
// granules -- in its own HBM, fine-grained so that a peer's system-scope loads see the owner's write-through stores, exports it as
// an IPC handle, and maps its peers' areas.  A rank writes only its own area (local stores) and polls the others' (reads over
// xGMI between the GPUs of a node; plain device memory between two processes on one GPU).  The tags of the granules tell runs
// apart, so the area is zeroed once, here.
SmgpuGatherXchg* smgpu_gather_xchg_new_device(uint32_t world, uint32_t rank, uint64_t rowcap) {
    return landing<SmgpuGatherXchg*>([&]() -> SmgpuGatherXchg* {
        if (world == 0 || world > GATHER_PEERS_MAX || rank >= world || rowcap == 0) throw err_internal("gather exchange (device): bad geometry");
        std::unique_ptr<GatherXchg> x(new GatherXchg());
        x->device = true;
        x->world = world; x->rank = rank; x->rowcap = rowcap;
        x->bytes = (((size_t)8 + (size_t)2 * rowcap) * 8 + 4095) & ~(size_t)4095;
        void* p = nullptr;
        hipError_t e = hipExtMallocWithFlags(&p, x->bytes, hipDeviceMallocFinegrained);
        if (e != hipSuccess) { (void)hipGetLastError(); throw err_internal(std::string("gather exchange (device): fine-grained allocation failed: ") + hipGetErrorString(e)); }
        x->own = (unsigned long long*)p;
        hip_check(hipMemset(x->own, 0, x->bytes), "memset");
        hip_check(hipDeviceSynchronize(), "sync");
        x->peers.assign(world, nullptr);
        x->peers[rank] = x->own;
        return reinterpret_cast<SmgpuGatherXchg*>(x.release());
    });
}
uintptr_t smgpu_gather_xchg_ipc_handle_size(void) { return sizeof(hipIpcMemHandle_t); }
void smgpu_gather_xchg_ipc_export(const SmgpuGatherXchg* xp, uint8_t* handle_out) {
    landing_void([&] {
        const GatherXchg* x = reinterpret_cast<const GatherXchg*>(xp);
        if (!x->device) throw err_internal("gather exchange: not a device-memory exchange");
        hipIpcMemHandle_t h;
        hip_check(hipIpcGetMemHandle(&h, x->own), "hipIpcGetMemHandle");
        memcpy(handle_out, &h, sizeof(h));
    });
}
void smgpu_gather_xchg_ipc_open(SmgpuGatherXchg* xp, uint32_t peer_rank, const uint8_t* handle) {
    landing_void([&] {
        GatherXchg* x = reinterpret_cast<GatherXchg*>(xp);
        if (!x->device || peer_rank >= x->world) throw err_internal("gather exchange: bad peer");
        if (peer_rank == x->rank) return;
        hipIpcMemHandle_t h;
        memcpy(&h, handle, sizeof(h));
        void* p = nullptr;
        hip_check(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
        x->opened.push_back(p);
        x->peers[peer_rank] = (unsigned long long*)p;
    });
}
bool smgpu_gather_xchg_is_device(const SmgpuGatherXchg* xp) { return reinterpret_cast<const GatherXchg*>(xp)->device; }
void smgpu_gather_xchg_free(SmgpuGatherXchg* p) { delete reinterpret_cast<GatherXchg*>(p); }
bool smgpu_gather_loop_eligible(const SmgpuGather* p, uint32_t n_wg) {
    return gather_loop_eligible(reinterpret_cast<const GatherRaw*>(p)->g, n_wg);
}
void smgpu_gather_loop_reserve(SmgpuGather* p, uint32_t n_wg, uint64_t rowcap, void* stream) {
    landing_void([&] { hip_check(gather_loop_reserve(reinterpret_cast<GatherRaw*>(p)->g, (hipStream_t)stream, n_wg, rowcap), "loop memory"); });
}
// enqueue the armed loop of this rank's shard (nothing is waited for: smgpu_gather_results reads it back)
bool smgpu_gather_launch_shared(SmgpuGather* p, SmgpuGatherXchg* xp, uint32_t rank, uint32_t run_id, uint32_t n_wg, void* stream) {
    return landing<bool>([&]() -> bool {
        GatherDev& g = reinterpret_cast<GatherRaw*>(p)->g;
        GatherXchg* x = reinterpret_cast<GatherXchg*>(xp);
        GatherShared sh;
        sh.rec = x->dev;
        sh.rows = x->dev ? x->dev + (size_t)2 * x->world * 4 : nullptr;
        sh.W = x->world; sh.rank = rank; sh.rowcap = x->rowcap; sh.run_id = run_id;
        if (x->device) {
            if (rank != x->rank) throw err_internal("gather exchange (device): this area belongs to another rank");
            for (uint32_t r = 0; r < x->world; ++r)
                if (!x->peers[r]) throw err_internal("gather exchange (device): the area of rank " + std::to_string(r) + " was never opened");
            sh.peers = x->peers.data();
        }
        if (g.longest_row > x->rowcap) throw err_internal("gather exchange: a row of this shard is longer than the exchange's slots");
        bool ran = false;
        hip_check(gather_launch_loop(g, (hipStream_t)stream, n_wg, &sh, &ran), "gather loop (shared)");
        return ran;
    });
}
void smgpu_debug_hold_cus(uint32_t n_wg, uint32_t lds_bytes, uint64_t micros, void* stream) {
    landing_void([&] { hip_check(debug_hold_cus(n_wg, lds_bytes, micros, (hipStream_t)stream), "hold CUs"); });
}
void smgpu_debug_qindex_find(const uint64_t* d_query, uint64_t nq, const uint64_t* d_probes, uint64_t n, int32_t form,
                             uint32_t* d_pos_out, void* stream) {
    landing_void([&] { hip_check(debug_qindex_find(d_query, nq, d_probes, n, form, d_pos_out, (hipStream_t)stream), "query index probe"); });
}
uint64_t smgpu_gather_longest_row(const SmgpuGather* p) { return reinterpret_cast<const GatherRaw*>(p)->g.longest_row; }
void smgpu_gather_topk_export_raw(SmgpuGather* p, uint64_t* d_records, uint32_t k, uint64_t stride, void* stream) {
    landing_void([&] {
        hip_check(gather_topk_export(reinterpret_cast<GatherRaw*>(p)->g, d_records, k, stride, (hipStream_t)stream), "top-k export");
    });
}
void smgpu_gather_cands_load_raw(SmgpuGather* p, const uint64_t* d_records, uint32_t n_records, uint64_t stride, void* stream) {
    landing_void([&] {
        hip_check(gather_cands_load(reinterpret_cast<GatherRaw*>(p)->g, d_records, n_records, stride, (hipStream_t)stream),
                  "candidate load");
    });
}
void smgpu_gather_replay_raw(SmgpuGather* p, uint32_t rounds, void* stream) {
    landing_void([&] {
        hip_check(gather_replay_rounds(reinterpret_cast<GatherRaw*>(p)->g, rounds, (hipStream_t)stream), "replay");
    });
}
uint64_t smgpu_gather_poll(SmgpuGather* p, bool* done, void* stream) {
    return landing<uint64_t>([&]() -> uint64_t {
        GatherDev& g = reinterpret_cast<GatherRaw*>(p)->g;
        unsigned long long head[GS_SLOTS];
        hip_check(hipMemcpyAsync(head, g.state, sizeof(head), hipMemcpyDeviceToHost, (hipStream_t)stream), "D2H");
        hip_check(hipStreamSynchronize((hipStream_t)stream), "sync");
        if (done) *done = head[GS_DONE] != 0;
        return head[GS_ROUNDS];
    });
}
uint64_t smgpu_gather_results(SmgpuGather* p, uint64_t* out_index, uint64_t* out_isect, uint64_t cap, void* stream) {
    return landing<uint64_t>([&]() -> uint64_t {
        GatherDev& g = reinterpret_cast<GatherRaw*>(p)->g;
        hipStream_t st = (hipStream_t)stream;
        unsigned long long head[GS_SLOTS];
        hip_check(hipMemcpyAsync(head, g.state, sizeof(head), hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        if (head[GS_ERR]) {
            // codes 10-14: the loop gave up between two rounds (at its gate, or waiting for a workgroup or a rank) and the index is
            // intact -- the caller agrees with its peers on what to do next (parallel.gather_distributed: the record protocol)
            const unsigned long long code = head[GS_ERR];
            if (gather_loop_gave_up(code)) { hip_check(hipMemsetAsync(g.state + GS_ERR, 0, 8, st), "memset"); g.loop_fallbacks++; }
            throw err_internal("gather loop: a workgroup or rank waited too long for its peers (code " + std::to_string(code) + ", epoch " +
                               std::to_string(head[13]) + ", workgroup " + std::to_string(head[14]) + ")");
        }
        const uint64_t n = head[GS_ROUNDS], m = n < cap ? n : cap;
        if (m) {
            hip_check(hipMemcpyAsync(out_index, g.out_idx, m * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipMemcpyAsync(out_isect, g.out_isect, m * 8, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
        }
        return n;
    });
}

void smgpu_overlap_raw(const uint64_t* d_query, uint64_t nq, const uint64_t* d_hashes, const uint64_t* d_offsets,
                       uint64_t ndb, uint64_t* d_overlap, int32_t op, void* stream) {
    landing_void([&] {
        hip_check(overlap_vector_launch(d_query, nq, d_hashes, d_offsets, ndb, (unsigned long long*)d_overlap, op,
                                        (hipStream_t)stream), "overlap");
    });
}
void smgpu_argmax_raw(const uint64_t* d_overlap, uint64_t ndb, uint64_t index_base, uint64_t* d_best, void* stream) {
    landing_void([&] {
        hip_check(argmax_launch((const unsigned long long*)d_overlap, ndb, index_base, (unsigned long long*)d_best,
                                (hipStream_t)stream), "argmax");
    });
}
uint64_t smgpu_intersect_workspace_bytes(uint64_t n) { return (uint64_t)select_temp_bytes(n) + ((n + 255) / 256) * 256 + 256; }

void smgpu_intersect_raw(const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* d_out, uint64_t* d_n,
                         void* d_ws, uint64_t ws_bytes, void* stream) {
    select_pair(d_a, na, d_b, nb, d_out, d_n, d_ws, ws_bytes, 0, stream);
}
void smgpu_subtract_raw(const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* d_out, uint64_t* d_n,
                        void* d_ws, uint64_t ws_bytes, void* stream) {
    select_pair(d_a, na, d_b, nb, d_out, d_n, d_ws, ws_bytes, 1, stream);
}

}  // extern "C"
