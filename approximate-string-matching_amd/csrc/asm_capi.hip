// C ABI of libasm_mi355x.so (declared in include/asm_mi355x.h): handle/stream management, device-resident
// batches, kernel dispatch.  Host side is C++17 compiled by hipcc; nothing here computes alignments on the
// CPU — without a HIP device every compute entry point returns ASM_ENODEVICE.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <fcntl.h>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <type_traits>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "../../include/asm_mi355x.h"
#include "asm_launch.h"
#include "asm_plan.h"
#include "asm_host.h"
#include "asm_kernels.h"
#include "asm_greedy3_kernel.h"
#include "asm_wide.h"
#include "asm_wave.h"
#include "asm_group.h"
#include "asm_cover.h"
#include "asm_tails.h"
#include "asm_filter.h"
#include "asm_ingest.h"
#include "asm_map.h"
#include "asm_fastq.h"
#include "asm_sam.h"
#include "asm_bam.h"
#include "asm_fasta.h"

/* What asm_run_benchmark_async (asm_step.h) keeps from call to call: the library's three streams beside the caller's, the events
 * that order the four, and the bookkeeping of a run of pipelined (repack = 2 / 3) calls. */
struct StepPipe {
    hipStream_t side_stream = nullptr;    /* Greedy beside the NW -> LEAP chain */
    hipStream_t pack_stream = nullptr;    /* repack = 2 / 3: packs for this call while the previous call still aligns */
    hipStream_t acc_stream = nullptr;     /* repack = 3: NW -> LEAP -> counters of a call, the counters behind both of its chains */
    hipEvent_t ev_packed = nullptr, ev_fork = nullptr, ev_join = nullptr, ev_leap = nullptr;
    hipEvent_t ev_gate = nullptr;         /* repack = 2: the next call's pack starts behind this point of the current call */
    bool gate_set = false;
    hipEvent_t ev_tail = nullptr;         /* the end of the latest overlapped call (repack = 3), on acc_stream */
    bool tail_set = false;                /* there were such calls: join_into before other streams or the host rely on them; only a
                                             later call with repack != 3, which joins them into the caller's stream for good, clears it */
    hipEvent_t ev_out[2] = {nullptr, nullptr}; /* repack = 3: the counters of the call before last (same output arrays) are done */
    unsigned calls3 = 0;                  /* overlapped calls of this run: call c records ev_out[c & 1], call c + 2 waits for it */
    const void* last3_out[3] = {nullptr, nullptr, nullptr}; /* the output arrays of the previous overlapped call (misuse guard) */
    bool last3_valid = false;
    bool pipe_prev = false;               /* the previous call packed on pack_stream: it is ordered behind the caller's stream already */
    hipError_t open() { /* the streams in this order: the runtime deals its hardware queues out by it */
        for (hipStream_t* s : {&side_stream, &pack_stream, &acc_stream})
            if (hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking)) return e;
        for (hipEvent_t* ev : {&ev_packed, &ev_fork, &ev_join, &ev_leap, &ev_gate, &ev_tail, &ev_out[0], &ev_out[1]})
            if (hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) return e;
        return hipSuccess;
    }
    void close() { /* a partly opened one too */
        for (hipStream_t s : {side_stream, pack_stream, acc_stream})
            if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t ev : {ev_packed, ev_fork, ev_join, ev_leap, ev_gate, ev_tail, ev_out[0], ev_out[1]})
            if (ev) (void)hipEventDestroy(ev);
    }
    /* joins the overlapped calls into stream s: everything they enqueued is ordered before what s gets next */
    hipError_t join_into(hipStream_t s) const { return tail_set ? hipStreamWaitEvent(s, ev_tail, 0) : hipSuccess; }
    /* the misuse guard of repack = 3: would this call write an array the previous overlapped call's counters may still read? */
    bool names_previous_outputs(const void* nw, const void* leap, const void* greedy) const {
        return last3_valid && ((nw && nw == last3_out[0]) || (leap && leap == last3_out[1]) || (greedy && greedy == last3_out[2]));
    }
    /* Forgetting the run, in the halves its two callers need.  A call with repack != 3: the next overlapped call starts a new run */
    void end_overlapped_run() { last3_valid = false, calls3 = 0; }
    /* ... asm_pipeline_join_async: the next pipelined call forks from the caller's stream again, with any output set (calls3 goes on) */
    void rejoin_caller() { pipe_prev = false, last3_valid = false; }
};

struct asm_handle {
    unsigned long long serial = 0;        /* unique over the life of the process: a batch names its owner by (pointer, serial), so a
                                             new handle that happens to get a destroyed one's address is not taken for it */
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    unsigned long long* d_pair_queue = nullptr; /* chunk counter of the wave-per-pair Greedy kernel (PairQueue, asm_wave.h) */
    StepPipe pipe;                        /* asm_run_benchmark_async: the library's own streams and what orders them (asm_step.h) */
    hipEvent_t ev_switch = nullptr;       /* switch_stream: the new stream behind the old one */
    bool overlap = true;                  /* ASM_OVERLAP=0: everything on one stream */
    std::string err;
    int num_cus = 256;
    int refill_greedy = 8;                /* idle lanes a wave of the persistent Greedy kernels collects before it refills (1 … 32 measured: flat) */
    bool greedy_fast = true;              /* Greedy, k <= 3, unit penalties, GLOBAL: the straight-line pass with integer rank keys
                                             (asm_greedy3.h; ASM_GREEDY_FAST=0: the FP64 kernel) */
    /* its rank tables (66 KB each), one per (significance constants, K) seen so far.  A table is written once, before its first
     * kernel, and never again — a call with other parameters gets another table, so kernels of earlier, still running calls on
     * other streams keep reading theirs.  The newest is tried first. */
    struct G3Table {
        G3Sig sig;
        int k;
        bool ok;
        uint2* d;
    };
    std::vector<G3Table> g3_tables;
    const uint2* d_g3_table = nullptr;    /* the table of the current call (set by g3_prepare) */
    bool leap_hint = true;                /* LEAP scheduled by a work hint when one is given (ASM_LEAP_HINT=0 disables) */
    bool bucketing = true;                /* group mixed-length batches by width class (ASM_BUCKET=0 disables) */
    bool wave_kernels = true;             /* wave-per-pair kernels for 6 <= k <= 31 (ASM_WAVE=0: workgroup-per-pair LDS kernels) */
    bool nw_bylen = true;                 /* unit-cost NW on mixed-length batches: workgroup-local sort by length (ASM_NW_BYLEN=0) */
    bool nw_banded = true;                /* banded bit-parallel NW with in-kernel full-height recompute (ASM_NW_BANDED=0) */
    bool nw_pair2 = true;                 /* unit-cost NW on one-granule batches in input order: two pairs per thread in 16-row windows
                                             (ASM_NW_PAIR2=0: one pair per thread in a 32-row window) */
    bool nw_wfa = true;                   /* affine NW: banded wavefront first, full matrix for the rest (ASM_NW_WFA=0: full matrix only) */
    int64_t map_cand_cap = (int64_t)1 << 24; /* asm_map_reads: verification candidates per round (ASM_MAP_CAND_CAP) */
    int64_t map_chunk = (int64_t)1 << 18;    /* asm_map_reads: reads per device chunk (ASM_MAP_CHUNK) */
    int64_t map_run_cap = (int64_t)1 << 24;  /* asm_map_reads_all: run records reserved per seeding round (ASM_MAP_RUN_CAP) */
    int mapq_model = 0;                   /* asm_map_set_mapq_model: ASM_MAPQ_REFERENCE or ASM_MAPQ_GAP */
    std::vector<uint8_t> last_mapq;       /* asm_map_last_mapq: one byte per record slot of the last in-memory mapping call */
    bool last_mapq_valid = false;
    unsigned sam_tags = 0;                /* asm_map_set_sam_tags: the optional tags of the file calls' lines (ASM_SAM_TAG_MD) */
    int out_format = 0;                   /* asm_map_set_output_format: what the file calls write, ASM_OUT_SAM or ASM_OUT_BAM */
    int bgzf_level = 0;                   /* asm_map_set_bgzf_level: the BAM container's blocks, ASM_BGZF_STORED or ASM_BGZF_DEFLATE */
    int bam_index = 0;                    /* asm_map_set_bam_index: what the sorted BAM calls write beside the file, ASM_BAM_INDEX_NONE or _BAI */
    asm_bam_index_stats last_bai = {};    /* asm_map_last_bam_index: of the last sorted BAM call that wrote an index */
    std::vector<hipEvent_t> prof_ev;      /* asm_profile_enable: 8 events per recorded asm_run_benchmark_async call */
    std::vector<unsigned> prof_mask;      /* which of a call's four kernels were launched */
    int prof_cap = 0;
    unsigned prof_select = 0xfu;          /* which kernels are bracketed: bit 0 pack, 1 NW, 2 LEAP, 3 Greedy */
    uint8_t* d_sort = nullptr;            /* wide-band LEAP: keys, permutation and radix-sort scratch of the global work sort */
    size_t sort_cap = 0;                  /* in bytes */
    bool leap_sort = true;                /* ASM_LEAP_SORT=0: work-sort inside workgroups only */
    uint32_t* d_todo = nullptr;           /* affine NW: [0] = count, [1..] = bucket slots the wavefront band could not settle */
    size_t todo_cap = 0;
    /* Device memory of batches is recycled instead of freed: a streamed file, or the reference-shaped per-pair objects, create
     * and drop a batch per call, and hipMalloc / hipFree cost more than the kernels (hipFree also drains the device).  Blocks
     * are handed out again in stream order (everything a handle enqueues is ordered on its stream), so no wait is needed. */
    std::unordered_map<void*, size_t> pool_live;
    std::multimap<size_t, void*> pool_idle;
    size_t pool_idle_bytes = 0;
    bool pooling = true;                  /* ASM_POOL=0: plain hipMalloc / hipFree */
    /* pinned host memory of asm_stream_seq_file, kept between calls (pinning 200 MB costs as much as streaming it) */
    char* pin_raw[3] = {nullptr, nullptr, nullptr};
    size_t pin_raw_cap = 0;
    int32_t* pin_pen[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int64_t pin_pen_cap[2][3] = {{0, 0, 0}, {0, 0, 0}};
};

static size_t pool_round(size_t bytes) { /* eight size classes per octave, at least 4 KiB */
    if (bytes <= 4096) return 4096;
    int top = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t step = (size_t)1 << (top - 3);
    return (bytes + step - 1) & ~(step - 1);
}

static void pool_release_idle(asm_handle* h) {
    for (auto& kv : h->pool_idle) (void)hipFree(kv.second);
    h->pool_idle.clear();
    h->pool_idle_bytes = 0;
}

static hipError_t pool_alloc(asm_handle* h, void** p, size_t bytes) {
    if (!h->pooling) return hipMalloc(p, bytes ? bytes : 1);
    const size_t want = pool_round(bytes);
    auto it = h->pool_idle.lower_bound(want);
    if (it != h->pool_idle.end() && it->first <= want + want / 4) { /* a block of this class or slightly above */
        *p = it->second;
        h->pool_live[*p] = it->first;
        h->pool_idle_bytes -= it->first;
        h->pool_idle.erase(it);
        return hipSuccess;
    }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) { /* out of memory: give the idle blocks back and try once more */
        (void)hipGetLastError();
        pool_release_idle(h);
        e = hipMalloc(p, want);
    }
    if (e == hipSuccess) h->pool_live[*p] = want;
    return e;
}

/* hipMalloc for the scratch blocks that do not come from the pool (traceback cells, sort scratch, todo lists, ...): when the
 * device is full, the idle blocks of the pool (up to 24 GiB) are what is in the way — give them back and try once more. */
static hipError_t big_malloc(asm_handle* h, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess && h && !h->pool_idle.empty()) {
        (void)hipGetLastError();
        (void)hipDeviceSynchronize(); /* idle blocks may still be read by queued work */
        pool_release_idle(h);
        e = hipMalloc(p, bytes);
    }
    return e;
}

static void pool_free(asm_handle* h, void* p) {
    if (!p) return;
    if (!h || !h->pooling) {
        (void)hipFree(p);
        return;
    }
    auto it = h->pool_live.find(p);
    if (it == h->pool_live.end()) { /* not ours (allocated before pooling was switched, or by another handle) */
        (void)hipFree(p);
        return;
    }
    const size_t sz = it->second;
    h->pool_live.erase(it);
    if (h->pool_idle_bytes + sz > ((size_t)24 << 30)) { /* keep at most 24 GiB idle */
        (void)hipFree(p);
        return;
    }
    h->pool_idle.emplace(sz, p);
    h->pool_idle_bytes += sz;
}

/* A call-scoped pool block of handle h: back to h's pool when it goes out of scope. */
template <typename T>
struct Scratch {
    asm_handle* h;
    T* p = nullptr;
    explicit Scratch(asm_handle* owner) : h(owner) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { pool_free(h, p); }
    hipError_t alloc(size_t bytes) { return pool_alloc(h, (void**)&p, bytes); }
};

/* ... and a call-scoped block from big_malloc, outside the pool: freed when it goes out of scope. */
template <typename T>
struct BigScratch {
    T* p = nullptr;
    BigScratch() = default;
    BigScratch(const BigScratch&) = delete;
    BigScratch& operator=(const BigScratch&) = delete;
    ~BigScratch() { (void)hipFree(p); }
    hipError_t alloc(asm_handle* h, size_t bytes) { return big_malloc(h, (void**)&p, bytes); }
};

static thread_local std::string g_err;
/* handles that exist: a batch remembers the handle whose pool its device blocks came from, and may be freed through another
 * handle, or after its own is gone */
static std::mutex g_live_mu;
static std::vector<asm_handle*> g_live_handles;
static unsigned long long g_next_serial = 1; /* under g_live_mu */
/* call with g_live_mu held: is the handle that created a batch still the one living at that address? */
static bool owner_is_live_locked(const asm_handle* h, unsigned long long serial) {
    for (asm_handle* q : g_live_handles)
        if (q == h) return q->serial == serial;
    return false;
}

static int fail(asm_handle* h, int code, const std::string& msg) {
    g_err = msg;
    if (h) h->err = msg;
    return code;
}

#define HIPCHK(h, call)                                                                           \
    do {                                                                                          \
        hipError_t _e = (call);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            return fail(h, _e == hipErrorOutOfMemory ? ASM_ENOMEM : ASM_ENODEVICE,                \
                        std::string(#call) + ": " + hipGetErrorString(_e));                       \
        }                                                                                         \
    } while (0)

/* A kernel launch on the handle's stream (launch_on, asm_launch.h) and its error: one expression for HIPCHK / STREAM_TRY.  The
 * stream is always h->stream: the step scheduler reaches its other streams by borrowing that (StreamBorrow, asm_step.h). */
template <class... P, class... A>
static hipError_t launch_lds(asm_handle* h, void (*kernel)(P...), unsigned grid, unsigned block, size_t lds, A&&... args) {
    return launch_on(h->stream, kernel, grid, block, lds, std::forward<A>(args)...);
}
template <class... P, class... A>
static hipError_t launch(asm_handle* h, void (*kernel)(P...), unsigned grid, unsigned block, A&&... args) {
    return launch_on(h->stream, kernel, grid, block, 0, std::forward<A>(args)...);
}

static int grid_for(int64_t n) { return (int)((n + ASM_BLOCK - 1) / ASM_BLOCK); }

/* Run-time value -> template argument, the one way this library does it: fn(std::integral_constant<int, C>{}) for the first C
 * of Lo, Lo + 1, ..., Hi with v <= C; a value above Hi takes Hi.  The callee reads C as decltype(c)::value. */
template <int Lo, int Hi, class F>
static auto with_const(int v, F fn) {
    if constexpr (Lo < Hi) {
        if (v > Lo) return with_const<Lo + 1, Hi>(v, fn);
    }
    return fn(std::integral_constant<int, Lo>{});
}

/* ... and over a short ascending list: the first listed C with v <= C; a value above the last takes the last. */
template <int First, int... Rest, class F>
static auto with_const_of(int v, F fn) {
    if constexpr (sizeof...(Rest) > 0) {
        if (v > First) return with_const_of<Rest...>(v, fn);
    }
    return fn(std::integral_constant<int, First>{});
}

/* A grow-only device buffer of the handle: room for at least `need` elements behind p afterwards (what it held is not kept). */
template <class T>
static int grow_device(asm_handle* h, T*& p, size_t& cap, size_t need) {
    if (cap >= need) return ASM_OK;
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
    HIPCHK(h, big_malloc(h, (void**)&p, sizeof(T) * need));
    cap = need;
    return ASM_OK;
}

/* the batch: "scalars back, one wait" and hipcub's scratch, the batch and its owner, the builder behind every constructor, the pack
 * launch, the tail resolver's host side and the entries of batches and references */
extern "C" {
#include "asm_batch.h"
}

/* one(bucket, its OutMap onto `out`) for every width class of a batch, up to the first that fails */
template <class F>
static int for_each_bucket(const asm_batch* b, int32_t* out, F one) {
    for (int q = 0; q < b->nb; q++) {
        OutMap map;
        map.out = out;
        map.order = b->bk[q].order;
        if (const int rc = one(b->bk[q], map)) return rc;
    }
    return ASM_OK;
}

/* Rank table of the straight-line Greedy kernel for these significance constants (asm_greedy3.h): built on the host with the
 * reference build's three roundings, uploaded once per (constants, k).  False when the constants do not have the structure
 * the integer keys need (then the FP64 kernel runs). */
static bool g3_prepare(asm_handle* h, const GreedyArgs& ga, int K) {
    const G3Sig sig = {ga.sig_match, ga.sig_mismatch, ga.sig_indel};
    for (size_t q = h->g3_tables.size(); q-- > 0;) {
        const asm_handle::G3Table& t = h->g3_tables[q];
        if (t.k == K && memcmp(&sig, &t.sig, sizeof(sig)) == 0) {
            h->d_g3_table = t.d;
            return t.ok;
        }
    }
    /* a new parameter set: builds the table on the host and BLOCKS until it is on the device (once per parameter set) */
    asm_handle::G3Table t = {sig, K, false, nullptr};
    std::vector<uint2> tab;
    if (g3_build_table(sig, K, tab)) {
        if (h->g3_tables.size() >= 16) { /* a caller cycling through parameter sets: drop the oldest, after everything has drained */
            (void)hipDeviceSynchronize();
            if (h->g3_tables.front().d) (void)hipFree(h->g3_tables.front().d);
            h->g3_tables.erase(h->g3_tables.begin());
        }
        if (big_malloc(h, (void**)&t.d, sizeof(uint2) * G3_TABLE_ENTRIES) == hipSuccess &&
            hipMemcpyAsync(t.d, tab.data(), sizeof(uint2) * G3_TABLE_ENTRIES, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
            hipStreamSynchronize(h->stream) == hipSuccess) { /* pageable source: staged before the call returns */
            t.ok = true;
        } else {
            (void)hipGetLastError();
            if (t.d) (void)hipFree(t.d);
            t.d = nullptr;
        }
    }
    h->g3_tables.push_back(t);
    h->d_g3_table = t.d;
    return t.ok;
}

extern "C" {

const char* asm_version(void) { return "asm_mi355x 0.1 (gfx950)"; }

void asm_default_params(asm_params* p) {
    if (!p) return;
    p->k = 3; /* benchmark.cpp:22 */
    p->x = p->o = p->e = 1;
    p->p_match = 0.80; /* hurdle_matrix.h:557-559 */
    p->p_mismatch = 0.20 / 3;
    p->p_indel = 0.40 / 3;
    p->alignment_type = ASM_ALIGN_GLOBAL; /* hurdle_matrix.h:553 default; the harness never passes another */
    p->leap_mode = ASM_LEAP_GLOBAL;
}

int asm_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

/* Releases everything a handle holds — a partly created one too — and the handle itself. */
static void handle_teardown(asm_handle* h) {
    (void)hipSetDevice(h->device);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    h->pipe.close();
    if (h->d_pair_queue) (void)hipFree(h->d_pair_queue);
    if (h->d_sort) (void)hipFree(h->d_sort);
    if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
    if (h->d_todo) (void)hipFree(h->d_todo);
    for (auto& t : h->g3_tables)
        if (t.d) (void)hipFree(t.d);
    for (hipEvent_t ev : h->prof_ev) (void)hipEventDestroy(ev);
    (void)hipDeviceSynchronize();
    for (char* q : h->pin_raw)
        if (q) (void)hipHostFree(q);
    for (auto& row : h->pin_pen)
        for (int32_t* q : row)
            if (q) (void)hipHostFree(q);
    pool_release_idle(h);
    for (auto& kv : h->pool_live) (void)hipFree(kv.first); /* batches the caller never freed */
    delete h;
}

int asm_create(asm_handle** out, int device) {
    if (!out) return fail(nullptr, ASM_EINVAL, "asm_create: out is NULL");
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0)
        return fail(nullptr, ASM_ENODEVICE, "asm_create: no HIP device is visible (this library has no CPU path)");
    if (device < 0 || device >= c) return fail(nullptr, ASM_EINVAL, "asm_create: device index out of range");
    std::unique_ptr<asm_handle, void (*)(asm_handle*)> owned(new asm_handle, handle_teardown); /* released on every early return */
    asm_handle* const h = owned.get();
    h->device = device;
    HIPCHK(h, hipSetDevice(device));
    HIPCHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    HIPCHK(h, h->pipe.open());
    HIPCHK(h, hipMalloc((void**)&h->d_pair_queue, sizeof(unsigned long long)));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, device));
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    /* The switches the library keeps (read once, here): one fallback per kernel family, the allocator, and the stream layout.
     * Everything else that used to be switchable was an A/B whose outcome is recorded in DESIGN.md. */
    const char* env;
    if ((env = getenv("ASM_OVERLAP"))) h->overlap = env[0] != '0';         /* 0: asm_run_benchmark_async on one stream */
    if ((env = getenv("ASM_LEAP_HINT"))) h->leap_hint = env[0] != '0';     /* 0: LEAP in input order (no work sort) */
    if ((env = getenv("ASM_LEAP_SORT"))) h->leap_sort = env[0] != '0';     /* 0: wide-band LEAP sorts inside workgroups only */
    if ((env = getenv("ASM_BUCKET"))) h->bucketing = env[0] != '0';        /* 0: mixed-length batches in one width class */
    if ((env = getenv("ASM_WAVE"))) h->wave_kernels = env[0] != '0';       /* 0: workgroup-per-pair fallbacks (asm_wide.h) */
    if ((env = getenv("ASM_POOL"))) h->pooling = env[0] != '0';            /* 0: plain hipMalloc / hipFree */
    if ((env = getenv("ASM_NW_BANDED"))) h->nw_banded = env[0] != '0';     /* 0: full-height bit-parallel NW */
    if ((env = getenv("ASM_NW_BYLEN"))) h->nw_bylen = env[0] != '0';       /* 0: mixed-length NW without the length sort */
    if ((env = getenv("ASM_NW_PAIR2"))) h->nw_pair2 = env[0] != '0';       /* 0: one-granule NW with one pair per thread */
    if ((env = getenv("ASM_NW_WFA"))) h->nw_wfa = env[0] != '0';           /* 0: affine NW by the full matrix only */
    if ((env = getenv("ASM_GREEDY_FAST"))) h->greedy_fast = env[0] != '0'; /* 0: FP64 Greedy kernel at k <= 3 */
    if ((env = getenv("ASM_MAP_CAND_CAP")) && atoll(env) > 0) h->map_cand_cap = atoll(env); /* smaller: more seeding rounds */
    if ((env = getenv("ASM_MAP_CHUNK")) && atoll(env) > 0) h->map_chunk = atoll(env);
    if ((env = getenv("ASM_MAP_RUN_CAP")) && atoll(env) > 0) h->map_run_cap = atoll(env); /* smaller: the buffer grows more often */
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        h->serial = g_next_serial++;
        g_live_handles.push_back(h);
    }
    *out = owned.release();
    return ASM_OK;
}

int asm_destroy(asm_handle* h) {
    if (!h) return ASM_OK;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        for (size_t i = 0; i < g_live_handles.size(); i++)
            if (g_live_handles[i] == h) {
                g_live_handles.erase(g_live_handles.begin() + (long)i);
                break;
            }
    }
    handle_teardown(h);
    return ASM_OK;
}

const char* asm_last_error(const asm_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

/* The pool recycles freed blocks in the order of the handle's stream.  When that stream changes, work queued on the old one may
 * still use blocks that are live now and go back to the pool later (or are idle already): everything enqueued under the new
 * stream is therefore ordered behind everything enqueued so far on the old one — an event, no host wait. */
static int switch_stream(asm_handle* h, hipStream_t next) {
    if (next == h->stream) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventRecord(h->ev_switch, h->stream));
    HIPCHK(h, hipStreamWaitEvent(next, h->ev_switch, 0));
    HIPCHK(h, h->pipe.join_into(next)); /* overlapped calls end on the library's own streams */
    h->stream = next;
    return ASM_OK;
}

int asm_set_stream(asm_handle* h, void* hip_stream) {
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_set_stream: NULL handle");
    /* NULL is HIP's legacy default stream (what torch.cuda.current_stream().cuda_stream is outside a stream context): work is
     * then ordered with everything else the caller enqueues there.  The handle's own stream is non-blocking — it never
     * synchronises with the legacy stream — so it is only restored on request (asm_reset_stream). */
    return switch_stream(h, (hipStream_t)hip_stream);
}

int asm_reset_stream(asm_handle* h) {
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_reset_stream: NULL handle");
    return switch_stream(h, h->own_stream);
}

int asm_synchronize(asm_handle* h) {
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_synchronize: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->pipe.tail_set) HIPCHK(h, hipStreamSynchronize(h->pipe.acc_stream)); /* calls with repack = 3 end on the library's own streams */
    return ASM_OK;
}

/* ---------------------------------------------------------------------------------------------------- */
int asm_generate_pairs(const asm_gen_config* cfg, int64_t first, int64_t n, uint32_t* read_off, uint32_t* ref_off,
                       char* reads, size_t reads_cap, char* refs, size_t refs_cap) {
    std::string err;
    const int rc = asm_host::generate_pairs(cfg, first, n, read_off, ref_off, reads, reads_cap, refs, refs_cap, err);
    return rc ? fail(nullptr, rc, err) : ASM_OK;
}

/* ---------------------------------------------------------------------------------------------------- */
/* the parameter rules (check_params_rule, asm_plan.h) on this library's error path */
static int check_params(asm_handle* h, int aligner, const asm_params* p, int maxlen = ASM_MAX_LENGTH) {
    const ParamVerdict v = check_params_rule(aligner, p, maxlen);
    return v.code ? fail(h, v.code, v.msg) : ASM_OK;
}

/* the aligners and the filters: launchers, align_bucket / align_batch, coverage, SIMD_ED and SHD (decisions: asm_plan.h) */
#include "asm_align_host.h"

int asm_count_equal_async(asm_handle* h, const int32_t* d_a, const int32_t* d_b, int64_t n, unsigned long long* d_count) {
    if (!h || !d_a || !d_b || !d_count) return fail(h, ASM_EINVAL, "asm_count_equal_async: NULL argument");
    if (n <= 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int64_t blocks = (n + ASM_BLOCK - 1) / ASM_BLOCK;
    if (blocks > 512) blocks = 512;
    HIPCHK(h, launch(h, count_equal_kernel, (unsigned)blocks, ASM_BLOCK, d_a, d_b, (long)n, d_count));
    return ASM_OK;
}

int asm_accuracy_async(asm_handle* h, const int32_t* d_nw, const int32_t* d_leap, const int32_t* d_greedy,
                       const int32_t* d_answers, int64_t n, unsigned long long* d_counters) {
    if (!h || !d_counters) return fail(h, ASM_EINVAL, "asm_accuracy_async: NULL argument");
    if (n <= 0) return ASM_OK;
    if ((((uintptr_t)d_nw | (uintptr_t)d_leap | (uintptr_t)d_greedy | (uintptr_t)d_answers) & 15u) != 0)
        return fail(h, ASM_EINVAL, "asm_accuracy_async: penalty arrays must be 16-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    int64_t blocks = (n / 4 + ASM_BLOCK - 1) / ASM_BLOCK;
    /* every workgroup ends with three atomics on one cache line, and a hot line takes only ~90 atomics/us: 977 workgroups
     * made this kernel 38 us at 10^6 pairs (rocprof, round 1); 128 grid-striding workgroups keep the loads wide enough */
    blocks = blocks < 1 ? 1 : (blocks > 128 ? 128 : blocks);
    if (!d_nw && !d_answers) blocks = 1; /* nothing to compare with: total_tests only */
    HIPCHK(h, launch(h, accuracy_kernel, (unsigned)blocks, ASM_BLOCK, d_nw, d_leap, d_greedy, d_answers, (long)n, d_counters));
    return ASM_OK;
}

#include "asm_step.h" /* asm_run_benchmark_async, asm_pipeline_join_async, asm_profile_enable / asm_profile_read */

#include "asm_stream.h"

/* ---------------------------------------------------------------------------------------------------- */
/* Streaming ingest: a `>read\n<ref\n` file (benchmark_utils.h:325-352) through the aligners in chunks.
 *   reader threads   pread() the next chunk into pinned host memory (three buffers in rotation) and count its newlines, so
 *                    that the chunk ends on a pair boundary; what follows the boundary is carried into the next chunk
 *   copy stream      raw bytes -> HBM (two device buffers), overlapped with the compute stream's work on the chunk before
 *   compute stream   parse on the device (asm_ingest.h), pack, [sequential mode: chain the stale tails from the state the
 *                    chunks before left behind], NW / LEAP / Greedy, counters, penalties back into pinned staging
 *   caller's thread  hands results of chunk c-2 to the caller's arrays while chunk c-1 computes and chunk c is copied */
#define SEQ_TRY(call) STREAM_TRY("asm_stream_seq_file", call)

extern "C++" {
/* Result staging of asm_stream_seq_file on the device: penalties and answers per device buffer, and "the chunk's results are in
 * pinned memory".  The destructor waits for the device (the aligners run on the library's own streams too) before it frees. */
struct SeqStaging {
    asm_handle* h;
    int32_t* d_pen[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int32_t* d_ans[2] = {nullptr, nullptr};
    hipEvent_t ev_done[2] = {nullptr, nullptr};
    explicit SeqStaging(asm_handle* owner) : h(owner) {}
    ~SeqStaging() {
        (void)hipDeviceSynchronize();
        for (int q = 0; q < 2; q++) {
            if (ev_done[q]) (void)hipEventDestroy(ev_done[q]);
            for (int a = 0; a < 3; a++) pool_free(h, d_pen[q][a]);
            pool_free(h, d_ans[q]);
        }
    }
};
}

int asm_stream_seq_file(asm_handle* h, const char* path, const asm_params* p, int greedy_mode, int aligner_mask,
                        int64_t chunk_bytes, int64_t max_pairs, int32_t* nw, int32_t* leap, int32_t* greedy, int64_t out_cap,
                        const int32_t* answers, int64_t n_answers, asm_stream_stats* stats) {
    if (!h || !path || !p || !stats) return fail(h, ASM_EINVAL, "asm_stream_seq_file: NULL argument");
    if (greedy_mode != ASM_GREEDY_CLEAN && greedy_mode != ASM_GREEDY_SEQUENTIAL)
        return fail(h, ASM_EINVAL, "asm_stream_seq_file: unknown greedy_mode");
    memset(stats, 0, sizeof *stats);
    const bool do_nw = (aligner_mask & 1) != 0, do_leap = (aligner_mask & 2) != 0, do_greedy = (aligner_mask & 4) != 0;
    if (!(do_nw || do_leap || do_greedy)) return fail(h, ASM_EINVAL, "asm_stream_seq_file: empty aligner mask");
    HIPCHK(h, hipSetDevice(h->device));
    StreamInput in(h, "asm_stream_seq_file");
    size_t file_bytes = 0;
    if (const int rc = in.open_file(path, &file_bytes)) return rc;
    size_t chunk = chunk_bytes > 0 ? (size_t)chunk_bytes : ((size_t)64 << 20);
    chunk = chunk < 4096 ? 4096 : chunk;
    if (chunk > ((size_t)1 << 30)) chunk = (size_t)1 << 30;
    const size_t slot_cap = chunk + ((size_t)4 << 20); /* + room for the carried tail and the EOF padding */
    /* reader workers: one thread's page-cache copy (~5 GB/s) is far below PCIe; a GPU box gives a job 16 CPUs per GPU */
    int reader_threads = (int)std::thread::hardware_concurrency();
    reader_threads = reader_threads > 16 ? 16 : (reader_threads < 2 ? 2 : reader_threads);
    if (const char* env = getenv("ASM_READER_THREADS")) reader_threads = atoi(env) > 0 ? atoi(env) : reader_threads;
    const auto t_begin = std::chrono::steady_clock::now();

    if (h->pin_raw_cap < slot_cap) { /* (re)pin */
        for (char*& q : h->pin_raw) {
            if (q) (void)hipHostFree(q);
            q = nullptr;
        }
        h->pin_raw_cap = 0;
        for (char*& q : h->pin_raw) SEQ_TRY(hipHostMalloc((void**)&q, slot_cap + 64, hipHostMallocDefault));
        h->pin_raw_cap = slot_cap;
    }
    for (int q = 0; q < 3; q++) in.pin[q] = h->pin_raw[q]; /* borrowed: they stay on the handle */
    SEQ_TRY(in.open_device(slot_cap, true, false));
    Scratch<unsigned long long> d_cnt(h);
    BatchPtr chunk_batch[2];
    SeqStaging st(h); /* declared behind what it must outlive: its destructor waits for the device before anything is given back */
    for (hipEvent_t& ev : st.ev_done) SEQ_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    SEQ_TRY(d_cnt.alloc(32));
    SEQ_TRY(hipMemsetAsync(d_cnt.p, 0, 32, h->stream));
    /* the reader side lives in asm_host.h (no HIP there: the same code runs under ThreadSanitizer in host/asm_host_check.cpp);
     * the one thing it needs from the device is "has the copy out of this slot finished".  Large chunks ramp up from a sixteenth:
     * the transfer of the first chunk starts after 1/16 of a chunk has been read instead of after a whole one */
    const size_t first_chunk = chunk >= ((size_t)32 << 20) ? chunk / 16 : chunk;
    asm_host::ChunkReader<asm_host::PairsFill> rd(chunk, first_chunk, in.wait_shipped(), in.fd, file_bytes, reader_threads, max_pairs);
    for (int q = 0; q < 3; q++) rd.slot[q].buf = in.pin[q], rd.slot[q].cap = slot_cap;
    rd.start();

    /* ---- caller's thread: ship, compute, harvest ---- */
    uint8_t tail_state[256];
    memset(tail_state, 0, sizeof tail_state);
    int64_t chunk_first[2] = {0, 0}, chunk_pairs[2] = {0, 0};
    int64_t pen_cap = 0; /* device staging is (re)allocated with the first chunk; the pinned side is reused when large enough */
    int64_t done_pairs = 0, chunks = 0;
    size_t bytes_total = 0;
    int maxlen = 0;
    auto harvest = [&](int q) -> int { /* results of the chunk that used device buffer q */
        if (chunk_pairs[q] <= 0 && !chunk_batch[q]) return ASM_OK;
        if (hipEventSynchronize(st.ev_done[q]) != hipSuccess) return fail(h, ASM_ENODEVICE, "asm_stream_seq_file: chunk failed");
        int32_t* dst[3] = {nw, leap, greedy};
        for (int a = 0; a < 3; a++) {
            if (!dst[a] || !h->pin_pen[q][a]) continue;
            const int64_t room = out_cap - chunk_first[q];
            const int64_t cnt = chunk_pairs[q] < room ? chunk_pairs[q] : (room > 0 ? room : 0);
            if (cnt > 0) memcpy(dst[a] + chunk_first[q], h->pin_pen[q][a], sizeof(int32_t) * (size_t)cnt);
        }
        chunk_batch[q].reset();
        chunk_pairs[q] = 0;
        return ASM_OK;
    };
    auto process = [&](int q, size_t shipped, int64_t n, int64_t) -> int { /* the chunk whose text sits in d_raw[q] */
        if (const int rc = harvest(q)) return rc; /* the chunk two back used the same result staging */
        if (n > pen_cap) { /* staging sized from the first chunk for a full one (its pairs per byte, times the slot's bytes, plus an
                              eighth: chunks ramp up to `chunk`); pen_cap = 0 until the first chunk — not "is the NW buffer there",
                              which a mask without NW never satisfies */
            if (const int rc = harvest(q ^ 1)) return rc;
            const int64_t full = (int64_t)((double)n / (double)(shipped ? shipped : 1) * (double)slot_cap) + 1;
            const int64_t cap = (full > n ? full : n) + (full > n ? full : n) / 8 + 1024;
            for (int qq = 0; qq < 2; qq++)
                for (int a = 0; a < 3; a++) {
                    if (!((aligner_mask >> a) & 1)) continue;
                    pool_free(h, st.d_pen[qq][a]);
                    st.d_pen[qq][a] = nullptr;
                    if (!h->pin_pen[qq][a] || h->pin_pen_cap[qq][a] < cap) {
                        if (h->pin_pen[qq][a]) (void)hipHostFree(h->pin_pen[qq][a]);
                        h->pin_pen[qq][a] = nullptr, h->pin_pen_cap[qq][a] = 0;
                        SEQ_TRY(hipHostMalloc((void**)&h->pin_pen[qq][a], sizeof(int32_t) * (size_t)cap, hipHostMallocDefault));
                        h->pin_pen_cap[qq][a] = cap;
                    }
                    SEQ_TRY(pool_alloc(h, (void**)&st.d_pen[qq][a], sizeof(int32_t) * (size_t)cap));
                }
            for (int qq = 0; qq < 2 && answers; qq++) {
                pool_free(h, st.d_ans[qq]);
                st.d_ans[qq] = nullptr;
                SEQ_TRY(pool_alloc(h, (void**)&st.d_ans[qq], sizeof(int32_t) * (size_t)cap));
            }
            pen_cap = cap;
        }
        BatchPtr b;
        if (const int rc = batch_new(h, n, ASM_GREEDY_CLEAN, "asm_stream_seq_file", b)) return rc;
        if (const int rc = batch_from_device_text(h, in.d_raw[q], shipped, b.get())) return rc;
        if (greedy_mode == ASM_GREEDY_SEQUENTIAL && do_greedy) { /* the chain of hurdle_matrix.h:136-137 across chunk boundaries */
            uint8_t summary[256]; /* the summary does not depend on the state the tails are resolved from */
            b->greedy_mode = ASM_GREEDY_SEQUENTIAL;
            if (const int rc = batch_resolve_tails(h, b.get(), tail_state, summary, true)) return rc;
            if (const int rc = asm_batch_pack_async(h, b.get())) return rc;
            if (const int rc = asm_tail_state_advance(tail_state, summary, n)) return rc;
        }
        const int32_t* ans = nullptr;
        if (answers && done_pairs < n_answers) { /* read_answer_file (benchmark_utils.h:358-368): one integer per pair */
            const int64_t have = n_answers - done_pairs < n ? n_answers - done_pairs : n;
            std::vector<int32_t> pad((size_t)n, INT32_MIN);
            memcpy(pad.data(), answers + done_pairs, sizeof(int32_t) * (size_t)have);
            SEQ_TRY(hipMemcpyAsync(st.d_ans[q], pad.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
            SEQ_TRY(hipStreamSynchronize(h->stream)); /* `pad` is pageable and about to go out of scope */
            ans = st.d_ans[q];
        }
        if (const int rc = asm_run_benchmark_async(h, b.get(), p, 0, do_nw ? st.d_pen[q][0] : nullptr, do_leap ? st.d_pen[q][1] : nullptr,
                                                   do_greedy ? st.d_pen[q][2] : nullptr, ans, d_cnt.p))
            return rc;
        for (int a = 0; a < 3; a++)
            if (st.d_pen[q][a])
                SEQ_TRY(hipMemcpyAsync(h->pin_pen[q][a], st.d_pen[q][a], sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        SEQ_TRY(hipEventRecord(st.ev_done[q], h->stream));
        maxlen = b->maxlen > maxlen ? b->maxlen : maxlen;
        chunk_batch[q] = std::move(b), chunk_first[q] = done_pairs, chunk_pairs[q] = n;
        done_pairs += n, bytes_total += shipped, chunks++;
        return ASM_OK;
    };
    if (const int rc = in.run(rd, "asm_stream_seq_file: read failed (or one pair is longer than a chunk)",
                              [](const asm_host::ChunkSlot&, int64_t) { return ASM_OK; }, process))
        return rc;
    for (int q = 0; q < 2; q++)
        if (const int rc = harvest(q)) return rc;
    SEQ_TRY(hipStreamSynchronize(h->stream));
    SEQ_TRY(hipMemcpy(stats->counters, d_cnt.p, 32, hipMemcpyDeviceToHost));
    rd.stop();
    stats->pairs = done_pairs, stats->chunks = chunks, stats->bytes = (int64_t)bytes_total, stats->max_length = maxlen;
    stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    stats->seconds_read = rd.read_seconds();
    return ASM_OK;
}
#undef SEQ_TRY

/* ---- read mapping: host side in csrc/asm_map_host.h (kernels: csrc/asm_map.h, design: docs/design/mapper.md) -------------------- */
#include "asm_map_host.h"
/* the BGZF container of the file calls' BAM output: frame kernel, record stream, asm_bgzf_frame */
#include "asm_bgzf.h"
/* the container read back: the deflate decoder, bgzf_inflate_kernel, asm_bgzf_decompress */
#include "asm_inflate.h"
/* the output side of the file calls: MapOutput (file, output slots, writer, record stream) and the report of a failed write */
#include "asm_map_out.h"
/* what the sorted file calls keep on the device, their sort and their gather */
#include "asm_sam_sort.h"
/* the BAI index beside a sorted BAM file, built from what the sort leaves on the device */
#include "asm_bai.h"
/* asm_map_file: FASTQ in, SAM out, through the same stages */
#include "asm_map_file.h"
/* asm_map_pairs_file: two FASTQ files in, paired SAM out */
#include "asm_map_pairs_file.h"
/* asm_index_build_file: FASTA in, index out */
#include "asm_index_file.h"

/* ---------------------------------------------------------------------------------------------------- */
int asm_device_malloc(asm_handle* h, size_t bytes, void** d_ptr) {
    if (!h || !d_ptr) return fail(h, ASM_EINVAL, "asm_device_malloc: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, pool_alloc(h, d_ptr, bytes ? bytes : 1));
    return ASM_OK;
}
int asm_device_free(asm_handle* h, void* d_ptr) {
    if (!h) return fail(h, ASM_EINVAL, "asm_device_free: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    pool_free(h, d_ptr); /* recycled in stream order: work already enqueued on the handle's stream may still use it */
    return ASM_OK;
}
int asm_memcpy_d2h(asm_handle* h, void* dst, const void* d_src, size_t bytes) {
    if (!h) return fail(h, ASM_EINVAL, "asm_memcpy_d2h: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return ASM_OK;
}
int asm_memcpy_h2d(asm_handle* h, void* d_dst, const void* src, size_t bytes) {
    if (!h) return fail(h, ASM_EINVAL, "asm_memcpy_h2d: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return ASM_OK;
}
int asm_memset_async(asm_handle* h, void* d_ptr, int value, size_t bytes) {
    if (!h) return fail(h, ASM_EINVAL, "asm_memset_async: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(d_ptr, value, bytes, h->stream));
    return ASM_OK;
}

struct asm_timer {
    hipEvent_t a = nullptr, b = nullptr;
    ~asm_timer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
int asm_timer_create(asm_handle* h, void** timer) {
    if (!h || !timer) return fail(h, ASM_EINVAL, "asm_timer_create: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    std::unique_ptr<asm_timer> t(new asm_timer);
    HIPCHK(h, hipEventCreate(&t->a));
    HIPCHK(h, hipEventCreate(&t->b));
    *timer = t.release();
    return ASM_OK;
}
int asm_timer_start(asm_handle* h, void* timer) {
    if (!h || !timer) return fail(h, ASM_EINVAL, "asm_timer_start: NULL argument");
    HIPCHK(h, hipEventRecord(((asm_timer*)timer)->a, h->stream));
    return ASM_OK;
}
int asm_timer_stop(asm_handle* h, void* timer) {
    if (!h || !timer) return fail(h, ASM_EINVAL, "asm_timer_stop: NULL argument");
    HIPCHK(h, hipEventRecord(((asm_timer*)timer)->b, h->stream));
    return ASM_OK;
}
int asm_timer_elapsed_ms(asm_handle* h, void* timer, float* ms) {
    if (!h || !timer || !ms) return fail(h, ASM_EINVAL, "asm_timer_elapsed_ms: NULL argument");
    asm_timer* t = (asm_timer*)timer;
    HIPCHK(h, hipEventSynchronize(t->b));
    HIPCHK(h, hipEventElapsedTime(ms, t->a, t->b));
    return ASM_OK;
}
int asm_timer_destroy(asm_handle* h, void* timer) {
    delete (asm_timer*)timer;
    (void)h;
    return ASM_OK;
}

} /* extern "C" */
