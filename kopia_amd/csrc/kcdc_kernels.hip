// MI355X (gfx950) kernels for Kopia's content-defined-chunking splitters.
//
// Reference semantics (bit-exact):
//   buzhash32Splitter.NextSplitPoint   repo/splitter/splitter_buzhash32.go:26-67
//   rabinKarp64Splitter.NextSplitPoint repo/splitter/splitter_rabinkarp64.go:26-67
//   fixedSplitter.NextSplitPoint       repo/splitter/splitter_fixed.go:15-26
//
// Key identity: the rolling hash is never reset inside a
// stream and always equals the hash of the 64 bytes ending at the current
// position (zero bytes before the stream start).  So cand(p) := hash(p) & mask
// == 0 is a pure function of bytes p-63..p, and the chunk rule is: from chunk
// start s, cut after the first p in [s+min-1, s+max-1] with cand(p), else after
// s+max-1.  The reference's fast path (only the last 64 of the first min-1
// bytes are rolled) becomes "start scanning at s+min-64": bytes before that are
// never read.
//
// Kernels, all in one translation unit with the host code below; one header per
// component, included in dependency order:
//   kcdc_split_config.h  the build switches KCDC_TRACE, KCDC_DEBUG_CHECKS, KCDC_HELP_DIAG
//   kcdc_split_base.h    wave and tile constants, roll3, uni64, byte_at, the Loader
//   kcdc_split_hash.h    buzhash32 and rabinkarp64 (BuzRing, Rabin), scan_region
//   kcdc_split_feed.h    BatchArgs, HashSmem, the LDS-DMA step slots and feed, TileGeom
//   kcdc_split_queue.h   agent-scope atomics, the queue header, PStream, tickets, take, steal, help slots
//   kcdc_split_visit.h   Visit, Tile, visit_*: the protocol between two tile scans
//   kcdc_split_buz.h     split_batch_pipe_kernel: the batch hot path (buzhash)
//   kcdc_split_rk.h      the Rabin-Karp tables, two-chain walk and split_batch_rk_kernel
//   kcdc_split_scan.h    init_ring, poison_counts, split_fixed, scan_first*, scan_server, fill_prng
//   kcdc_split_long.h    the long path: cand_scan_dma / cand_scan_rk, seg_prefix, compact, resolve
// Below them: device tables, queue workspaces, the batch plan, the launchers, the scan server's
// host side and the test hooks.  They share the per-device locks, g_test and the queue
// workspaces, and launch the kernels from template instantiations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>
#include <string>

#include "kcdc_hip.h"
#include "kcdc_internal.h"

#include "kcdc_split_config.h"
#include "kcdc_split_base.h"
#include "kcdc_split_hash.h"
#include "kcdc_split_feed.h"
#include "kcdc_split_queue.h"
#include "kcdc_split_visit.h"
#include "kcdc_split_buz.h"
#include "kcdc_split_rk.h"
#include "kcdc_split_scan.h"
#include "kcdc_split_long.h"

namespace kcdc {

// ================================================================== host
struct DeviceTables {
    uint32_t* buz = nullptr;
    uint64_t* rk_out = nullptr;
    uint64_t* rk_mod = nullptr;
    int cus = 0;
};

namespace {
constexpr int kMaxDevices = 64;
constexpr int kQueueSlots = 64;  // per-launch queue workspaces, chosen round-robin per launch
DeviceTables g_dev_tables[kMaxDevices];
// Queue workspace of one launch slot: header (256 B: head, tail, done, error words 64 B
// apart) | ring (P x 8 B, P = pow2 > nstreams + grid waves) | progress (nstreams x 24 B).
// Grow-only; a replaced buffer is freed once the slot's last launch (its `done` event) finished.
struct QueueWs {
    char* base = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;  // recorded after the slot's last launch: a reuse from another
                                // stream waits for it (more than kQueueSlots launches in flight)
    hipStream_t last = nullptr;  // the stream of the slot's last launch
    bool used = false;
};
QueueWs g_qws[kMaxDevices][kQueueSlots];
// Slot affinity: back-to-back launches on one stream reuse that stream's slot (stream order
// already serialises them, so no event wait, and the workspace stays warm); other streams
// take slots round-robin.  A few recent streams per device, least recently used replaced.
struct StreamSlot {
    hipStream_t st = nullptr;
    unsigned slot = 0;
    uint64_t tick = 0;
    bool valid = false;
};
constexpr int kStreamSlots = 8;
StreamSlot g_stream_slot[kMaxDevices][kStreamSlots];
uint64_t g_slot_tick[kMaxDevices];
bool g_dev_ready[kMaxDevices];
unsigned g_queue_next[kMaxDevices];
// Per-device locks: table setup and a launch's slot / workspace / enqueue sequence are
// serialised per device only, so threads driving different devices never wait on each other.
std::mutex g_dev_mu[kMaxDevices];

// Test hooks (kcdc_test_set, include/kcdc.h "testing"): read by every later launch.
struct TestKnobs {
    uint32_t spin_cap = 0;     // 0: dev::kSpinCap
    bool no_steal = false;     // disable try_steal
    bool force_error = false;  // mark every pipelined launch as failed
    int help = 0;              // intra-region help: 0 the policy below, 1 off, 2 on (A/B, tests)
    uint32_t lane_cap = 0;     // buzhash batch lane segment cap (256..4096, a power of two); 0: base_args' rule
    uint32_t help_window = 0;  // both batch kernels' help window in tiles (255: whole regions); 0: batch_plan's rule
    char* last_ws = nullptr;   // queue header of the last pipelined launch (kcdc_test_queue_stat)
    int last_dev = 0;
    uint32_t last_waves = 0;   // launch waves of that launch (kcdc_test_queue_stat key 12)
    uint64_t par_node_cap = 0; // long path: parallel-resolver nodes per launch; 0: kParNodeCap
    bool long_stat = false;    // long path: keep each launch's serial[] flags for kcdc_test_long_stat
    uint32_t* long_serial = nullptr;  // pinned host copy of the last long-path launch's serial[]
    uint32_t long_serial_cap = 0, long_streams = 0;
    bool long_seen = false;
};
TestKnobs g_test;

// Rotated buzhash frame for a reference mask (avg - 1).  A contiguous low mask of k bits
// (avg a power of two, the registered splitters) rotates to the top k bits: rot = 32 - k,
// and h & mask == 0 <=> h <= ~mask.  Any other mask keeps rot = 0 (top = false).
struct BuzFrame {
    uint32_t rot, mask, lim;
    bool top;
};
BuzFrame buz_frame(uint32_t mask) {
    BuzFrame f{0, mask, 0, false};
    if ((mask & (mask + 1u)) == 0) {  // 0b0..01..1 (including 0 and all ones)
        const uint32_t k = static_cast<uint32_t>(__builtin_popcount(mask));
        f.rot = (32u - k) & 31u;
        f.mask = f.rot ? (mask << f.rot) | (mask >> (32u - f.rot)) : mask;
        f.lim = ~f.mask;
        f.top = true;
    }
    return f;
}

uint32_t base_lane_cap(const Algo& algo, const TestKnobs& knobs) {
    // largest power of two <= avg / 256, within [256, kLaneMax]: tiles of ~avg/4 (1 MiB and
    // larger averages keep the full 2 KiB lane segments)
    uint64_t cap = algo.kind == kBuzhash ? dev::kBuzLaneMax : dev::kLaneMax;
    while (cap > 256 && cap * dev::kTileDiv > algo.avg) cap >>= 1;
    return algo.kind == kBuzhash && knobs.lane_cap ? knobs.lane_cap : static_cast<uint32_t>(cap);
}

dev::BatchArgs base_args(const Algo& algo, const DeviceTables& t) {
    dev::BatchArgs a{};
    a.min_size = algo.min_size();
    a.max_size = algo.max_size();
    a.mask = static_cast<uint32_t>(algo.mask());
    if (algo.kind == kBuzhash) {
        const BuzFrame f = buz_frame(a.mask);
        a.buz_rot = f.rot;
        a.mask = f.mask;
        a.buz_lim = f.lim;
    }
    a.buz = t.buz;
    a.rk_out = t.rk_out;
    a.rk_mod = t.rk_mod;
    a.rk_shift = static_cast<uint32_t>(tables().rk_shift);
    a.lane_cap = base_lane_cap(algo, g_test);
    return a;
}
#if KCDC_TRACE || KCDC_DEBUG_CHECKS
char* g_last_ws = nullptr;
#endif
#if KCDC_TRACE
uint64_t* g_trace = nullptr;
uint64_t g_trace_n = 0;
int trace_reserve(uint64_t nstreams) {
    if (g_trace_n >= nstreams) return 0;
    if (g_trace) (void)hipFree(g_trace);
    g_trace = nullptr;
    g_trace_n = 0;
    if (hipMalloc(&g_trace, 3 * 8 * nstreams) != hipSuccess) return -1;
    g_trace_n = nstreams;
    return 0;
}
#endif
}  // namespace

#if KCDC_TRACE || KCDC_DEBUG_CHECKS
// Trace / debug builds only: copy the last launch's queue header.
extern "C" int kcdc_debug_queue_copy(uint32_t* host) {  // the last launch's queue header
    if (!g_last_ws) return -22;
    return hipMemcpy(host, g_last_ws, dev::kQHeaderBytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;
}
#endif
#if KCDC_TRACE
extern "C" int kcdc_debug_trace_copy(uint64_t* host, uint64_t nstreams) {
    if (!g_trace || nstreams > g_trace_n) return -22;
    return hipMemcpy(host, g_trace, 3 * 8 * nstreams, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;
}
#endif

// Experiment switches that make the batch kernels cut WRONG: none are left in the source (round 4
// moved the timing ablations out; kcdc_version, tests/test_lib_host.py).
const char* ablations_kernels() { return ""; }

const DeviceTables* device_tables(int device, int* err) {
    *err = 0;
    if (device < 0 || device >= kMaxDevices) {
        *err = set_error(-22, "device index out of range");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_dev_mu[device]);
    if (g_dev_ready[device]) return &g_dev_tables[device];
    const Tables& T = tables();
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    if (e != hipSuccess) {
        *err = hip_error(e, "hipSetDevice");
        return nullptr;
    }
    DeviceTables d;
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) d.cus = prop.multiProcessorCount;
    if (e == hipSuccess) e = hipMalloc(&d.buz, sizeof(T.buz));
    if (e == hipSuccess) e = hipMalloc(&d.rk_out, sizeof(T.rk_out));
    if (e == hipSuccess) e = hipMalloc(&d.rk_mod, sizeof(T.rk_mod));
    if (e == hipSuccess) e = hipMemcpy(d.buz, T.buz, sizeof(T.buz), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.rk_out, T.rk_out, sizeof(T.rk_out), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.rk_mod, T.rk_mod, sizeof(T.rk_mod), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        *err = hip_error(e, "table upload");
        return nullptr;
    }
    g_dev_tables[device] = d;
    g_dev_ready[device] = true;
    return &g_dev_tables[device];
}

namespace {
// What a pipelined batch launch runs with: a pure function of the splitter, the stream count, the
// device's CUs and the test knobs.
struct BatchPlan {
    bool helpers;          // waiting waves help scan the owners' regions
    unsigned grid;         // workgroups (persistent: at most one per CU)
    unsigned wg_waves;     // waves per workgroup
    uint32_t lane_cap;     // BatchArgs::lane_cap
    uint32_t help_window;  // BatchArgs::help_window
    uint64_t ring;         // ring entries (a power of two)
    uint32_t hwaves;       // help slots: one per launch wave, none without helpers
    size_t ring_bytes, bytes;  // the ring's bytes; the whole workspace: header | ring | help area
};
BatchPlan batch_plan(const Algo& algo, uint32_t nstreams, unsigned cus, const TestKnobs& knobs) {
    BatchPlan p{};
    p.lane_cap = base_lane_cap(algo, knobs);
    const unsigned wg_waves = algo.kind == kRabinKarp ? dev::kRkWaves : dev::kDmaWaves;
    const unsigned need = (nstreams + wg_waves - 1) / wg_waves;
    // With helpers the batch kernels take the whole chip even for a few streams: the waves
    // without a stream help scan the owners' regions (help slots).  Help pays when a chunk's
    // test region spans many tiles: averages of 1 MiB and up (12+ buzhash tiles, 6+ Rabin-Karp
    // tiles per region).  Below that, the claims, row waits and helpers' polling cost more than
    // the tail they remove (same-process A/B, 4096 x 4 MiB: 128K-BUZHASH 3.42 vs 3.13 ms with
    // help off, 512K 2.37 vs 2.27; 64 x 64 MiB 128K-BUZHASH 27.5 vs 22.2 ms), except for the
    // Rabin-Karp kernel in launches with fewer streams than waves (64 x 64 MiB 128K-RABINKARP
    // 30.1 vs 38.0 ms); DESIGN.md §2.1d, profiles/r05/help_policy/.
    const bool helpers = knobs.help == 2 ||
                         (knobs.help == 0 &&
                          (algo.avg >= dev::kHelpMinAvg ||
                           (algo.kind == kRabinKarp && nstreams < static_cast<uint64_t>(cus) * wg_waves)));
    unsigned grid = helpers || need >= cus ? cus : need;
    if (grid > dev::kMaxPipeGrid) grid = dev::kMaxPipeGrid;  // one claim flag per workgroup
    // Fewer streams than waves: the waves without a stream of their own live on help tasks
    // (half tiles of the owners' regions), and 4 KiB buzhash lanes (tiles and help tasks twice
    // as long, half the claims, posts and warm-ups per region) win there, while with more
    // streams than waves they lose (the coarser tail).  Same-process A/B,
    // bit-exact, 2 KiB -> 4 KiB (profiles/r06/lane4k/): 4M 2048 x 8 MiB 1.864 -> 1.753 ms,
    // 1024 x 16 MiB 2.855 -> 2.516, 512 x 32 MiB 9.72 -> 7.69; 2M 1024 x 16 MiB 3.09 -> 2.84;
    // 1M loses at 2048 x 8 MiB (2.22 -> 2.29) and gains from 1024 x 16 MiB on (3.67 -> 3.61).
    if (algo.kind == kBuzhash && !knobs.lane_cap && p.lane_cap == dev::kBuzLaneMax && helpers &&
        nstreams * (algo.avg >= (2u << 20) ? 1u : 2u) <= static_cast<uint64_t>(grid) * wg_waves)
        p.lane_cap = 2 * dev::kBuzLaneMax;
    // Four or more waves per stream (both batch kernels): helpers outnumber the owners, and regions published
    // four tiles at a time keep them just ahead of the owner instead of on the far end of the
    // region (512 x 32 MiB 4M 7.83 -> 5.89 ms, 1M 8.28 -> 6.93).  With one helper per owner the
    // windows' re-publishing costs more than they save (1024 x 16 MiB 4M 2.49 -> 2.58 at 8
    // tiles, 3.10 at 4), so whole regions stay published there (profiles/r06/help_window/).
    if (knobs.help_window)
        p.help_window = knobs.help_window == 255u ? 0u : knobs.help_window;
    else if (helpers && 4u * nstreams <= static_cast<uint64_t>(grid) * wg_waves) {
        // buzhash: wider windows for more helpers per owner (16 waves per stream, 128 x 128 MiB:
        // W = 4 19.9 ms, 6 17.3, 8 18.8; 32 per stream, 64 x 256 MiB: 4 33.4, 6 30.4, 8 27.9)
        const uint64_t wps = static_cast<uint64_t>(grid) * wg_waves / nstreams;
        p.help_window = algo.kind == kBuzhash && wps >= 32 ? 8u : algo.kind == kBuzhash && wps >= 16 ? 6u : 4u;
    }
    // Rabin-Karp (a tile is ~2.5x a buzhash tile's time, so re-publishing costs relatively
    // less): windows of 8 tiles pay from one helper per owner on (1024 x 16 MiB 4M 4.52 ->
    // 4.05 ms, 1M 5.56 -> 5.46); with four or more, 4 tiles (512 x 32 MiB 8.17 -> 6.33,
    // 256 x 64 MiB 19.06 -> 11.69; profiles/r06/help_window/rk/)
    else if (algo.kind == kRabinKarp && helpers && 2u * nstreams <= static_cast<uint64_t>(grid) * wg_waves)
        p.help_window = 8u;
    uint64_t ring = 1;
    // every push (yields, tombstones) takes a fresh slot; a launch pushes at most
    // a few entries per wave beyond the initial n: size the ring with ample margin
    const uint64_t live = static_cast<uint64_t>(nstreams) + 8ull * grid * wg_waves;
    while (ring <= live) ring <<= 1;
    const size_t ring_bytes = static_cast<size_t>(dev::kPEntryStride) * ring;
    const uint32_t hwaves = helpers ? grid * wg_waves : 0u;
    const size_t help_bytes = static_cast<size_t>(hwaves) * (128u + 64u + 8u * dev::kHelpTiles) + 4u * ((hwaves + 31u) / 32u);
    p.helpers = helpers;
    p.grid = grid;
    p.wg_waves = wg_waves;
    p.ring = ring;
    p.hwaves = hwaves;
    p.ring_bytes = ring_bytes;
    p.bytes = dev::kQHeaderBytes + ring_bytes + help_bytes;
    return p;
}

// The queue workspace slot of a launch on stream st, with at least `bytes` bytes; call with
// g_dev_mu[device] held.  The slot is chosen by stream affinity (see StreamSlot) and grown
// stream-ordered; a launch that takes over a slot from another stream waits for the slot's
// last launch.
int queue_slot(int device, hipStream_t st, size_t bytes, QueueWs*& out) {
    unsigned slot = kQueueSlots;
    StreamSlot* aff = nullptr;
    for (StreamSlot& e : g_stream_slot[device]) {
        if (e.valid && e.st == st) aff = &e;
    }
    if (aff && g_qws[device][aff->slot].last == st) slot = aff->slot;
    if (slot == kQueueSlots) {
        slot = g_queue_next[device]++ % kQueueSlots;
        if (!aff) {  // remember this stream in the least recently used entry
            aff = &g_stream_slot[device][0];
            for (StreamSlot& e : g_stream_slot[device])
                if (!e.valid || e.tick < aff->tick) aff = &e;
            aff->valid = true;
            aff->st = st;
        }
        aff->slot = slot;
    }
    aff->tick = ++g_slot_tick[device];
    QueueWs& q = g_qws[device][slot];
    const bool same_stream = q.used && q.last == st;  // stream order covers the previous launch
    if (q.bytes < bytes) {
        DeviceGuard dg(device);
        char* nb = nullptr;
        size_t nbytes = bytes > 2 * q.bytes ? bytes : 2 * q.bytes;
        // Stream-ordered: a plain hipFree synchronises the whole device, so a launch that
        // grows its slot would wait for every kernel on every stream (tests/test_gpu_queue.py
        // steal test: the batch waited out a 300 ms occupier on another stream).
        hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&nb), nbytes, st);
        if (e == hipSuccess && q.base) {  // the slot's previous launches are the old buffer's only users
            if (q.done) e = hipStreamWaitEvent(st, q.done, 0);
            if (e == hipSuccess) e = hipFreeAsync(q.base, st);
        }
        if (e != hipSuccess) return hip_error(e, "queue workspace");
        q.base = nb;
        q.bytes = nbytes;
    }
    if (!q.done) {
        DeviceGuard dg(device);
        const hipError_t e = hipEventCreateWithFlags(&q.done, hipEventDisableTiming | hipEventDisableSystemFence);
        if (e != hipSuccess) return hip_error(e, "queue workspace event");
    } else if (!same_stream) {
        const hipError_t e = hipStreamWaitEvent(st, q.done, 0);
        if (e != hipSuccess) return hip_error(e, "queue workspace wait");
    }
    q.last = st;
    q.used = true;
    out = &q;
    return 0;
}

// launch(kind) with the hash kind of a rolling splitter as a compile-time constant: the KIND
// argument of the kernel templates is decltype(kind)::value.  FIXED splitters read no data.
template <class Launch>
int with_kind(const Algo& algo, const char* what, Launch launch) {
    if (algo.kind == kBuzhash)
        launch(std::integral_constant<int, kBuzhash>{});
    else if (algo.kind == kRabinKarp)
        launch(std::integral_constant<int, kRabinKarp>{});
    else
        return set_error(-22, std::string(what) + ": FIXED splitters read no data");
    return 0;
}

// After a kernel launch: 0, or the launch error recorded under `what`.
int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_error(e, what);
}
}  // namespace

int launch_split_batch(const Algo& algo, const SplitArgs& s, int device, void* stream) {
    int err = 0;
    const DeviceTables* t = device_tables(device, &err);
    if (!t) return err;
    if (s.nstreams == 0) return 0;
    dev::BatchArgs a = base_args(algo, *t);
    a.ptrs = s.ptrs;
    a.lens = s.lens;
    a.nstreams = s.nstreams;
    a.cuts = s.cuts;
    a.cuts_cap = s.cuts_cap;
    a.cut_base = s.cut_base;
    a.cut_end = s.cut_end;
    a.starts = s.starts;
    a.resume = s.starts ? s.resume : nullptr;
    a.counts = s.counts;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s.starts && algo.kind == kFixed) return set_error(-22, "per-stream starts need the pipelined batch kernels");
    if (algo.kind == kFixed) {
        hipLaunchKernelGGL(dev::split_fixed_kernel, dim3(s.nstreams), dim3(256), 0, st, a);
    } else {
        if (algo.kind == kRabinKarp && tables().rk_shift != 45)
            return set_error(-22, "Rabin-Karp kernel: the polynomial must have degree 53");
        const BatchPlan p = batch_plan(algo, s.nstreams, static_cast<unsigned>(t->cus), g_test);
        a.lane_cap = p.lane_cap;
        a.help_window = p.help_window;
        // The slot stays locked from its selection to its event record, so a later user of the
        // same slot always waits for this launch.
        std::lock_guard<std::mutex> lk(g_dev_mu[device]);
        QueueWs* q = nullptr;
        if (const int qe = queue_slot(device, st, p.bytes, q)) return qe;
        char* ws = q->base;
        a.queue = reinterpret_cast<uint32_t*>(ws);
        g_test.last_ws = ws;
        g_test.last_dev = device;
        g_test.last_waves = p.grid * p.wg_waves;
#if KCDC_TRACE || KCDC_DEBUG_CHECKS
        g_last_ws = ws;
#endif
        a.ring = reinterpret_cast<uint32_t*>(ws + dev::kQHeaderBytes);
        a.help = p.helpers ? reinterpret_cast<uint64_t*>(ws + dev::kQHeaderBytes + p.ring_bytes) : nullptr;
        a.help_waves = p.hwaves;
        a.ring_mask = static_cast<uint32_t>(p.ring - 1);

#if KCDC_TRACE
        if (trace_reserve(std::max<uint64_t>(s.nstreams, 5ull * p.grid * p.wg_waves)) != 0) return set_error(-12, "trace buffer");
        a.trace = g_trace;
#endif
        // header + ring zeroed per launch (the ring is also left empty by every finished launch)
        {
            const uint32_t slots = static_cast<uint32_t>(p.ring);
            const uint64_t threads = std::max<uint64_t>(std::max<uint64_t>(8ull * slots, dev::kQHeaderBytes / 4), p.hwaves);  // >= nstreams
            hipLaunchKernelGGL(dev::init_ring_kernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, st, a,
                               slots, p.grid * p.wg_waves, g_test.spin_cap ? g_test.spin_cap : dev::kSpinCap,
                               g_test.no_steal ? 0u : dev::kStealSpins);
        }
        // persistent grid: one workgroup per CU, never more workgroups than the streams need
        void (*kernel)(dev::BatchArgs) = algo.kind == kRabinKarp ? dev::split_batch_rk_kernel
                                         : buz_frame(static_cast<uint32_t>(algo.mask())).top
                                             ? dev::split_batch_pipe_kernel<true>
                                             : dev::split_batch_pipe_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.wg_waves * dev::kWave), 0, st, a);
        if (g_test.force_error)  // test hook: report a failed launch (kcdc_test_set)
            hipLaunchKernelGGL(dev::poison_counts_kernel, dim3(std::min<unsigned>((s.nstreams + 255) / 256, 256u)),
                               dim3(256), 0, st, a);
        const hipError_t er = hipEventRecord(q->done, st);
        if (er != hipSuccess) return hip_error(er, "queue workspace record");
    }
    return launched("split kernel launch");
}

int launch_scan_first(const Algo& algo, const uint8_t* d_buf, uint64_t len, int64_t lo, int64_t hi, int64_t* d_out,
                      int device, void* stream, uint8_t* d_scratch) {
    if (!d_scratch) return set_error(-22, "scan_first: no scratch buffer");
    int err = 0;
    const DeviceTables* t = device_tables(device, &err);
    if (!t) return err;
    dev::BatchArgs a = base_args(algo, *t);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = with_kind(algo, "scan_first", [&](auto kind) {
            hipLaunchKernelGGL(dev::scan_first_cp_kernel<decltype(kind)::value>, dim3(1),
                               dim3(dev::kScanWaves * dev::kWave), 0, st, a, d_buf, static_cast<int64_t>(len), lo, hi,
                               d_out, d_scratch);
        }))
        return rc;
    return launched("scan kernel launch");
}

// ---- resident scan server (host side): one per (device, hash kind)
namespace {
struct ScanServer {
    std::mutex mu;
    bool init = false;
    hipStream_t st = nullptr;
    dev::ServerMbox* h = nullptr;  // fine-grained, mapped
    dev::ServerMbox* d = nullptr;
    uint8_t* scratch = nullptr;
    uint64_t cap = 0;
    uint64_t seq = 0;
    bool launched = false;
    std::chrono::steady_clock::time_point last_answer{};  // the server was alive then
};
ScanServer g_srv[64][2];
bool g_srv_off = false;  // kcdc_test_set(KCDC_TEST_NO_SERVER)
std::atomic<uint64_t> g_srv_served{0};  // requests answered by a server (kcdc_test_server_requests)

int srv_launch(ScanServer& sv, const Algo& algo, const DeviceTables& t) {
    dev::BatchArgs a = base_args(algo, t);
    int rc = with_kind(algo, "scan server", [&](auto kind) {
        hipLaunchKernelGGL(dev::scan_server_kernel<decltype(kind)::value>, dim3(1), dim3(dev::kScanWaves * dev::kWave), 0,
                           sv.st, a, sv.d, sv.scratch, sv.seq - 1);
    });
    if (!rc) rc = launched("scan server launch");
    if (rc) return rc;
    sv.launched = true;
    return 0;
}
}  // namespace

void set_scan_server_off(bool off) { g_srv_off = off; }
uint64_t scan_server_requests() { return g_srv_served.load(std::memory_order_relaxed); }

int server_scan_first(const Algo& algo, const uint8_t* d_stage, uint64_t len, int64_t lo, int64_t hi, int device,
                      int64_t* out) {
    if (g_srv_off || device < 0 || device >= 64 || (algo.kind != kBuzhash && algo.kind != kRabinKarp)) return 1;
    ScanServer& sv = g_srv[device][algo.kind == kBuzhash ? 0 : 1];
    std::unique_lock<std::mutex> lk(sv.mu, std::try_to_lock);
    if (!lk.owns_lock()) return 1;  // another handle holds the server: the caller launches its own scan
    int err = 0;
    const DeviceTables* t = device_tables(device, &err);
    if (!t) return err;
    if (!sv.init) {
        if (hipStreamCreateWithFlags(&sv.st, hipStreamNonBlocking) != hipSuccess) return 1;
        void* p = nullptr;
        if (hipHostMalloc(&p, sizeof(dev::ServerMbox), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            return 1;
        sv.h = static_cast<dev::ServerMbox*>(p);
        std::memset(sv.h, 0, sizeof(dev::ServerMbox));
        void* pd = nullptr;
        if (hipHostGetDevicePointer(&pd, p, 0) != hipSuccess) return 1;
        sv.d = static_cast<dev::ServerMbox*>(pd);
        sv.init = true;
    }
    if (len > sv.cap) {  // grow the scratch: the previous server must be gone first
        if (sv.launched) {
            if (hipStreamSynchronize(sv.st) != hipSuccess) return hip_error(hipGetLastError(), "scan server sync");
            sv.launched = false;
        }
        if (sv.scratch) (void)hipFree(sv.scratch);
        sv.scratch = nullptr;
        sv.cap = 0;
        const uint64_t cap = std::max<uint64_t>((len + 255) & ~uint64_t(255), 4ull << 20);
        if (hipMalloc(&sv.scratch, cap) != hipSuccess) return 1;
        sv.cap = cap;
    }
    sv.h->src = reinterpret_cast<uint64_t>(d_stage);
    sv.h->len = static_cast<int64_t>(len);
    sv.h->lo = lo;
    sv.h->hi = hi;
    const uint64_t sq = ++sv.seq;
    __atomic_store_n(&sv.h->req_seq, sq, __ATOMIC_RELEASE);
    using clk = std::chrono::steady_clock;
    const auto t_start = clk::now();
    // A server that answered within the last millisecond is still polling (it idles out after
    // 2 ms): skip the runtime query, which costs microseconds.  Otherwise ask the stream.
    if (!sv.launched || (t_start - sv.last_answer > std::chrono::milliseconds(1) && hipStreamQuery(sv.st) == hipSuccess)) {
        const int rc = srv_launch(sv, algo, *t);
        if (rc) return rc;
    }
    // Wait for the answer.  A server that timed out before seeing this request has finished
    // its kernel (hipStreamQuery succeeds) without serving it: launch a new one.
    auto next_check = t_start + std::chrono::microseconds(200);
    uint32_t spins = 0;
    while (__atomic_load_n(&sv.h->done_seq, __ATOMIC_ACQUIRE) != sq) {
        if (++spins % 64 == 0) {
            const auto now = clk::now();
            if (now < next_check) continue;
            next_check = now + std::chrono::microseconds(200);
            if (hipStreamQuery(sv.st) == hipSuccess && __atomic_load_n(&sv.h->done_seq, __ATOMIC_ACQUIRE) != sq) {
                const int rc = srv_launch(sv, algo, *t);
                if (rc) return rc;
            }
            if (now - t_start > std::chrono::seconds(10)) return set_error(-5, "scan server did not answer");
        }
    }
    *out = __atomic_load_n(&sv.h->result, __ATOMIC_ACQUIRE);
    sv.last_answer = clk::now();
    g_srv_served.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

int launch_scan_first_batch(const Algo& algo, const uint8_t* d_base, const ScanReq* d_reqs, uint32_t n, int64_t* d_out,
                            int device, void* stream, uint8_t* d_scratch) {
    if (!d_scratch) return set_error(-22, "scan_first: no scratch buffer");
    int err = 0;
    const DeviceTables* t = device_tables(device, &err);
    if (!t) return err;
    if (n == 0) return 0;
    dev::BatchArgs a = base_args(algo, *t);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = with_kind(algo, "scan_first", [&](auto kind) {
            hipLaunchKernelGGL(dev::scan_first_batch_cp_kernel<decltype(kind)::value>, dim3(n),
                               dim3(dev::kScanWaves * dev::kWave), 0, st, a, d_base, d_reqs, d_out, d_scratch);
        }))
        return rc;
    return launched("scan kernel launch");
}

int launch_fill_prng(uint8_t* d_data, uint64_t stride, uint64_t stream_len, uint32_t nstreams, uint64_t seed,
                     uint64_t first_sid, void* stream) {
    if (stride % 8 != 0 || (nstreams > 1 && stride < stream_len))
        return set_error(-22, "fill_prng: stride must be a multiple of 8 and >= stream_len");
    if (nstreams == 0 || stream_len == 0) return 0;
    hipLaunchKernelGGL(dev::fill_prng_kernel, dim3(4096), dim3(256), 0, static_cast<hipStream_t>(stream), d_data,
                       stride, stream_len, nstreams, seed, first_sid);
    return launched("fill kernel launch");
}

namespace {
constexpr uint64_t kParNodeCap = uint64_t(1) << 20;  // parallel-resolver nodes per launch (<= 88 MB of tables)
struct LongLayout {
    int64_t nseg;
    uint64_t node_cap;
    uint32_t levels;
    size_t off_streams, off_cnt, off_cand, off_off, off_list, off_total, off_bsum, off_serial, off_forced, off_jump, bytes;
};
int64_t long_nseg(uint64_t len, uint64_t off0) {  // segments tile coordinates (position + off0)
    return len ? static_cast<int64_t>((len + off0 + dev::kSegBytes - 1) / dev::kSegBytes) : 0;
}
LongLayout long_layout(int64_t nseg, uint32_t nstreams) {
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    LongLayout L{};
    L.nseg = nseg;
    const size_t ns = static_cast<size_t>(nseg);
    size_t o = 0;
    L.off_streams = o;
    o += al(nstreams * sizeof(dev::LongStream));
    L.off_cnt = o;
    o += al(ns * 4);
    L.off_cand = o;
    o += al(ns * dev::kSegK * 8);
    L.off_off = o;
    o += al(ns * 8);
    L.off_list = o;
    o += al(ns * dev::kSegK * 8);
    L.off_total = o;
    o += 256;
    L.off_bsum = o;
    o += al((static_cast<size_t>(nseg) + dev::kPrefixItems - 1) / dev::kPrefixItems * 8 + 8);
    L.node_cap = 0;
    L.levels = 0;
    L.off_serial = L.off_forced = L.off_jump = o;
    {  // resolve_par_kernel for streams with complete candidate lists
        // (the test knob is read here, so the workspace size functions and the launch agree)
        L.node_cap = std::min<uint64_t>(static_cast<uint64_t>(ns) * dev::kSegK + 2ull * nstreams,
                                        g_test.par_node_cap ? g_test.par_node_cap : kParNodeCap);
        L.levels = 1;
        while ((uint64_t(1) << L.levels) <= L.node_cap) L.levels++;
        L.off_serial = o;
        o += al(nstreams * 4);
        L.off_forced = o;
        o += al(L.node_cap * 4);
        L.off_jump = o;
        o += al(static_cast<size_t>(L.levels) * L.node_cap * 4);
    }
    L.bytes = o;
    return L;
}
}  // namespace

size_t long_workspace_bytes(const Algo& algo, uint64_t len) {
    if (algo.kind == kFixed) return 0;
    return long_layout(long_nseg(len, 15), 1).bytes;  // any alignment: off0 < 16
}

size_t long_workspace_bytes_multi(const Algo& algo, const uint64_t* lens, uint32_t m) {
    if (algo.kind == kFixed) return 0;
    int64_t nseg = 0;
    for (uint32_t j = 0; j < m; j++) nseg += long_nseg(lens[j], 15);
    return long_layout(nseg, m).bytes;
}

int launch_split_long_multi(const Algo& algo, uint32_t m, const uint8_t* const* d_data, const uint64_t* lens,
                            uint64_t* const* d_cuts, const uint64_t* caps, uint64_t* const* d_counts, void* ws,
                            size_t ws_bytes, int device, void* stream) {
    int err = 0;
    const DeviceTables* t = device_tables(device, &err);
    if (!t) return err;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (algo.kind == kFixed)  // reads no data; the batch entry point covers it
        return set_error(-22, "long-stream path: use kcdc_split_batch_device for FIXED splitters");
    if (m == 0) return 0;
    std::vector<dev::LongStream> hs(m);
    int64_t nseg = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint64_t p = reinterpret_cast<uint64_t>(d_data[j]);
        dev::LongStream& S = hs[j];
        S.off0 = static_cast<int64_t>(p & 15u);
        S.abase = reinterpret_cast<const uint8_t*>(p - static_cast<uint64_t>(S.off0));
        S.n = static_cast<int64_t>(lens[j]);
        S.seg0 = nseg;
        S.cuts = d_cuts[j];
        S.cuts_cap = caps[j];
        S.count = d_counts[j];
        nseg += long_nseg(lens[j], static_cast<uint64_t>(S.off0));
    }
    const LongLayout L = long_layout(nseg, m);
    if (!ws || ws_bytes < L.bytes) return set_error(-22, "long-stream path: workspace too small");
    char* w = static_cast<char*>(ws);
    dev::LongArgs g{};
    g.streams = reinterpret_cast<const dev::LongStream*>(w + L.off_streams);
    g.nstreams = m;
    g.nseg = nseg;
    g.seg_cnt = reinterpret_cast<uint32_t*>(w + L.off_cnt);
    g.seg_cand = reinterpret_cast<uint64_t*>(w + L.off_cand);
    g.seg_off = reinterpret_cast<uint64_t*>(w + L.off_off);
    g.list = reinterpret_cast<uint64_t*>(w + L.off_list);
    g.total = reinterpret_cast<uint64_t*>(w + L.off_total);
    {
        g.serial = reinterpret_cast<uint32_t*>(w + L.off_serial);
        g.forced = reinterpret_cast<uint32_t*>(w + L.off_forced);
        g.jump = reinterpret_cast<uint32_t*>(w + L.off_jump);
        g.node_cap = L.node_cap;
        g.levels = L.levels;
    }
    hipError_t e = hipMemcpyAsync(w + L.off_streams, hs.data(), m * sizeof(dev::LongStream), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_error(e, "long-stream descriptors");
    dev::BatchArgs a = base_args(algo, *t);
    const int64_t mn = static_cast<int64_t>(algo.min_size()), mx = static_cast<int64_t>(algo.max_size());
    if (nseg > 0) {
        if (algo.kind == kBuzhash) {  // LDS-DMA fed, persistent: one workgroup per CU
            const dim3 pgrid(static_cast<unsigned>(
                std::min<int64_t>(t->cus, (nseg + dev::kDmaWaves - 1) / dev::kDmaWaves)));
            if (buz_frame(static_cast<uint32_t>(algo.mask())).top)
                hipLaunchKernelGGL(dev::cand_scan_dma_kernel<true>, pgrid, dim3(dev::kDmaWaves * dev::kWave), 0, st, a, g);
            else
                hipLaunchKernelGGL(dev::cand_scan_dma_kernel<false>, pgrid, dim3(dev::kDmaWaves * dev::kWave), 0, st, a, g);
        } else {  // Rabin-Karp: two-chain LDS-DMA tiles, persistent
            const dim3 pgrid(static_cast<unsigned>(
                std::min<int64_t>(t->cus, (nseg + dev::kRkWaves - 1) / dev::kRkWaves)));
            hipLaunchKernelGGL(dev::cand_scan_rk_kernel, pgrid, dim3(dev::kRkWaves * dev::kWave), 0, st, a, g);
        }
        const unsigned nblk = static_cast<unsigned>((nseg + dev::kPrefixItems - 1) / dev::kPrefixItems);
        uint64_t* bsum = reinterpret_cast<uint64_t*>(w + L.off_bsum);
        hipLaunchKernelGGL(dev::seg_blocksum_kernel, dim3(nblk), dim3(1024), 0, st, g, bsum);
        hipLaunchKernelGGL(dev::block_offsets_kernel, dim3(1), dim3(64), 0, st, g, bsum, nblk);
        hipLaunchKernelGGL(dev::seg_prefix_kernel, dim3(nblk), dim3(1024), 0, st, g, bsum);
        hipLaunchKernelGGL(dev::compact_kernel, dim3(static_cast<unsigned>((nseg + 255) / 256)), dim3(256), 0, st, g);
    }
    if (g.serial) {  // streams it cannot take (truncated segments) stay flagged for resolve_kernel
        if (nseg == 0) {
            e = hipMemsetAsync(w + L.off_total, 0, sizeof(uint64_t), st);
            if (e != hipSuccess) return hip_error(e, "long-stream total");
        }
        hipLaunchKernelGGL(dev::resolve_par_kernel, dim3(m), dim3(1024), 0, st, g, mn, mx);
    }
    int rc = with_kind(algo, "long-stream path", [&](auto kind) {
        hipLaunchKernelGGL(dev::resolve_kernel<decltype(kind)::value>, dim3(m), dim3(dev::kWave), 0, st, a, g, mn, mx);
    });
    if (!rc) rc = launched("long-stream kernel launch");
    if (rc) return rc;
    if (g_test.long_stat) {  // test hook: which resolver took each stream (kcdc_test_long_stat)
        if (m > g_test.long_serial_cap) {
            if (g_test.long_serial) {  // (an earlier launch's copy may still be in flight)
                (void)hipDeviceSynchronize();
                (void)hipHostFree(g_test.long_serial);
            }
            g_test.long_serial = nullptr;
            g_test.long_serial_cap = 0;
            e = hipHostMalloc(reinterpret_cast<void**>(&g_test.long_serial), m * sizeof(uint32_t), hipHostMallocDefault);
            if (e != hipSuccess) return hip_error(e, "long-stream statistics");
            g_test.long_serial_cap = m;
        }
        // stream-ordered after resolve_par_kernel, before the caller can release the workspace
        e = hipMemcpyAsync(g_test.long_serial, w + L.off_serial, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return hip_error(e, "long-stream statistics");
        g_test.long_streams = m;
        g_test.long_seen = true;
    }
    return 0;
}

int launch_split_long(const Algo& algo, const uint8_t* d_data, uint64_t len, uint64_t* d_cuts, uint64_t cuts_cap,
                      uint64_t* d_count, void* ws, size_t ws_bytes, int device, void* stream) {
    return launch_split_long_multi(algo, 1, &d_data, &len, &d_cuts, &cuts_cap, &d_count, ws, ws_bytes, device,
                                   stream);
}

// ------------------------------------------------------------------ testing
uint32_t& test_chunk_grid() {
    static uint32_t cap = 0;
    return cap;
}

extern "C" int64_t kcdc_test_server_requests(void) { return static_cast<int64_t>(scan_server_requests()); }

extern "C" int kcdc_test_set(int32_t key, int64_t value) {
    switch (key) {
        case 1: g_test.spin_cap = static_cast<uint32_t>(value); return 0;   // KCDC_TEST_SPIN_CAP
        case 2: g_test.no_steal = value != 0; return 0;                     // KCDC_TEST_NO_STEAL
        case 3: g_test.force_error = value != 0; return 0;                  // KCDC_TEST_FORCE_ERROR
        case 4: test_hash_lanes() = static_cast<int>(value); return 0;     // KCDC_TEST_HASH_LANES
        case 5: set_scan_server_off(value != 0); return 0;                 // KCDC_TEST_NO_SERVER
        case 6: g_test.help = value == 2 ? 2 : value != 0; return 0;       // KCDC_TEST_NO_HELP (2: force help on)
        case 7: test_id_ring_bytes() = static_cast<uint64_t>(value); return 0;  // KCDC_TEST_ID_RING
        case 8:                                                            // KCDC_TEST_LANE_CAP
            if (value != 0 && (value < 256 || value > 4096 || (value & (value - 1)) != 0))
                return set_error(-22, "lane cap: 0, or a power of two in [256, 4096]");
            g_test.lane_cap = static_cast<uint32_t>(value);
            return 0;
        case 9:                                                            // KCDC_TEST_HELP_WINDOW
            static_assert(dev::kHelpMinTiles == 3, "the range in the error text below");
            if (value < 0 || (value != 0 && (value < static_cast<int64_t>(dev::kHelpMinTiles) || value > 255)))
                return set_error(-22, "help window: 0 (policy), 255 (whole regions), or tiles in [3, 254]");
            g_test.help_window = static_cast<uint32_t>(value);
            return 0;
        case 10:                                                           // KCDC_TEST_PAR_NODE_CAP
            if (value < 0 || static_cast<uint64_t>(value) > kParNodeCap)
                return set_error(-22, "parallel-resolver node cap: 0 (default), or nodes in [1, 2^20]");
            g_test.par_node_cap = static_cast<uint64_t>(value);
            return 0;
        case 11: g_test.long_stat = value != 0; return 0;                  // KCDC_TEST_LONG_STAT
        case 12: return test_set_deflate_limit(false, value);              // KCDC_TEST_DEFLATE_MAXB
        case 13: return test_set_deflate_limit(true, value);               // KCDC_TEST_DEFLATE_CL_MAXB
        case 14:                                                           // KCDC_TEST_CHUNK_GRID
            if (value < 0) return set_error(-22, "chunk grid: 0 (default), or workgroups >= 1");
            test_chunk_grid() = static_cast<uint32_t>(value < 0x7fffffff ? value : 0x7fffffff);  // above any grid
            return 0;
        default: return set_error(-22, "unknown test knob");
    }
}

extern "C" int64_t kcdc_test_long_stat(int32_t key) {
    if (key != 1 && key != 2) return set_error(-22, "unknown long-stream statistic");
    if (!g_test.long_seen) return set_error(-22, "no long-stream launch recorded (KCDC_TEST_LONG_STAT)");
    if (key == 1) return static_cast<int64_t>(g_test.long_streams);
    int64_t serial = 0;
    for (uint32_t j = 0; j < g_test.long_streams; j++) serial += g_test.long_serial[j] != 0;
    return serial;
}

extern "C" int64_t kcdc_test_queue_stat(int32_t key) {
    if (key == 12) return g_test.last_ws ? static_cast<int64_t>(g_test.last_waves) : set_error(-22, "no pipelined batch launch yet");
    const int word = key == 1 ? dev::kQErr : key == 2 ? dev::kQDone : key == 3 ? dev::kQSteal : key == 4 ? dev::kQHelp
                   : key >= 5 && key <= 9 ? dev::kQDiag + (key - 5)
                   : key == 10 ? dev::kQHT : key == 11 ? dev::kQHT + 1 : -1;
    if (word < 0) return set_error(-22, "unknown queue statistic");
    if (!g_test.last_ws) return set_error(-22, "no pipelined batch launch yet");
    DeviceGuard dg(g_test.last_dev);
    uint32_t v = 0;
    const hipError_t e = hipMemcpy(&v, g_test.last_ws + 4 * word, 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? static_cast<int64_t>(v) : hip_error(e, "queue statistic");
}

// Test hook: what batch_plan gives a launch of `nstreams` streams of splitter `name` on device 0
// with the knobs as they stand -- out = {lane_cap, helpers, help_window, launch waves}.  Host only:
// the tests' geometry model (tests/batch_model.py) checks its lane cap against this.
extern "C" int kcdc_test_batch_plan(const char* name, uint32_t nstreams, uint32_t out[4]) {
    const Algo* algo = name ? find_algo(name) : nullptr;
    if (!algo || !out) return set_error(-22, "batch plan: unknown splitter or null output");
    if (algo->kind != kBuzhash && algo->kind != kRabinKarp) return set_error(-22, "batch plan: not a pipelined splitter");
    if (nstreams == 0) return set_error(-22, "batch plan: no streams");
    int err = 0;
    const DeviceTables* t = device_tables(0, &err);
    if (!t) return err;
    const BatchPlan p = batch_plan(*algo, nstreams, static_cast<unsigned>(t->cus), g_test);
    out[0] = p.lane_cap;
    out[1] = p.helpers ? 1u : 0u;
    out[2] = p.help_window;
    out[3] = p.grid * p.wg_waves;
    return 0;
}

// Test hook: bytes [off, off + n) of the last pipelined launch's queue workspace (header, ring,
// help slots) to host memory, for post-mortems of a launch (tools/batch_probe.py).
extern "C" int kcdc_test_ws_copy(void* dst, uint64_t off, uint64_t n) {
    if (!g_test.last_ws) return set_error(-22, "no pipelined batch launch yet");
    DeviceGuard dg(g_test.last_dev);
    const hipError_t e = hipMemcpy(dst, g_test.last_ws + off, n, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : hip_error(e, "workspace copy");
}

extern "C" int kcdc_test_occupy(uint32_t nwg, uint32_t usec, void* stream) {
    if (nwg == 0) return 0;
    if (usec > 10u * 1000u * 1000u) return set_error(-22, "occupy: at most 10 s");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dev::occupy_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return hip_error(e, "occupy attribute");
    uint32_t* sink = nullptr;
    e = hipMallocAsync(reinterpret_cast<void**>(&sink), 4, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_error(e, "occupy sink");
    hipLaunchKernelGGL(dev::occupy_kernel, dim3(nwg), dim3(64), 160 * 1024, static_cast<hipStream_t>(stream),
                       static_cast<uint64_t>(usec) * 100u, sink);
    e = hipGetLastError();
    (void)hipFreeAsync(sink, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_error(e, "occupy launch");
}

}  // namespace kcdc
