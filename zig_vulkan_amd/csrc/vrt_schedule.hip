// vrt_schedule.hip — the cost-feedback tile schedule (vrt::TileSchedule, vrt_ctx.h), all of it in one place: the kernel that sorts the
// tiles by their measured cost, a context's tile order and its buffers (schedule_create), where the traversal kernels find them
// (schedule_bind), which of its two rules serves a frame (schedule_frame), the re-sorts and the order of the second stream's frames
// against them.  Nothing else knows the buffers' layout, which order is current, or the events.
// tile_order 5 re-sorts the tile schedule in place before every frame on the primary stream: a frame running on
// the second stream would read it while it is being rewritten, so that order runs one frame at a time.  The
// amortised form, tile_order 7, sorts into the other of two buffers and may use both streams.
// (order_auto: frames that alternate between the two streams of a frames_in_flight = 2 context take reverse raster (3)
// instead, see schedule_frame, do_dispatch and DESIGN.md §4)
// The cost schedule's two rules (index 1: frames whose split tiles trace their second sample on the idle lanes — two samples per
// pixel — where a split costs nothing but the second workgroup's fixed part): how many tiles an order may split (cap), and the wave
// slots the "time the frame needs anyway" is computed for (slots); mode: the rule the current order was sorted under.
//   d_tile_cost      [half][tile][wave] cycles / 64, written by every frame of a scheduled kernel
//   d_tile_schedule  order 0, order 1 (`stride` entries each, XCD-major: 8 rows), then the snapshot of the costs and the split state (a
//                    word per tile each).  Frames read order `cur` (TraceParams::tile_schedule); an amortised sort writes the other one.
//   ev_sched         recorded on the primary stream behind sort number `seq`: a second-stream frame that has not seen that sort waits
//   ev_b_sched       recorded on the second stream behind its first frame after a sort: what it read from the OTHER order is finished;
//                    the next sort, which rewrites that order, waits for it
// What a sort computes is the kernel's comment; it affects timing only, never pixels.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>
#include "vrt_ctx.h"

namespace vrt {

// Cost-feedback schedule: order[] = owned tile ids in kScheduleBuckets classes of cost (wave-cycles of the most
// recent frame, relative to the maximum), heaviest class first; INSIDE a class the tiles keep the default
// reverse-raster order, so that consecutive workgroups still render neighbouring tiles (a full sort by cost
// measured 6-7 % slower on views without outliers: neighbouring tiles share the lines of the bitmaps they walk).
// With extra > 0 the tiles whose slowest wave would outlast the rest of the frame (longer than 1.25 x the frame's
// wave-cycles spread over all wave slots) are SPLIT: two entries, each renders half of the tile with 32 lanes per
// wave, in a class of their own at the front; at most `extra` tiles, unused spare entries are ~0.  snap[n .. 2n)
// remembers which tiles are split (their measured waves are scaled back up by 1.28 before the test, the measured
// gain of splitting, so that a split tile does not flip back and forth).
// One workgroup.  cost[] ([half][tile][wave], overwritten by every frame) is condensed into snap[] first: frames
// on another stream may still be writing cost[], and every pass below must see the same values or order[] would
// not be a permutation.  The order affects timing only, never pixels.
// Round 4: the halves of split tiles are no longer ONE class in reverse-raster order but kSplitBuckets classes by the tile's slowest
// wave, slowest first — on the reference app's own run nearly every tile that holds terrain is split (3 000 half-tile workgroups for
// 1 024 workgroup slots), and with them unordered the second generation of workgroups held waves as long as the first's longest:
// they started at 100 us and ended at 300 (tools/experiments/timeline_tail.py).
constexpr uint32_t kScheduleBuckets = 8u;
constexpr uint32_t kSplitBuckets = 8u;
constexpr uint32_t kAllBuckets = kScheduleBuckets + kSplitBuckets;
__global__ __launch_bounds__(1024) void vrt_schedule_kernel(const uint32_t *__restrict__ cost, uint32_t *__restrict__ snap,
                                                            const uint32_t *prev_order, uint32_t *order, uint32_t n, uint32_t extra_max,
                                                            uint32_t extra, uint32_t wave_slots) {
    __shared__ uint32_t s_max, s_nsplit, s_longest;
    __shared__ unsigned long long s_total;
    __shared__ uint32_t wave_total[kAllBuckets][16];
    __shared__ uint32_t class_total[kAllBuckets];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t *state = snap + n;
    // order[] is stored XCD-major: entry k at (k % 8) * row + k / 8.  extra_max: the spare entries the buffer holds (its layout);
    // extra <= extra_max: how many tiles this sort may split (the frames launch n + extra workgroups)
    const uint32_t row = (n + extra_max + 7u) >> 3;
    if (tid == 0) {
        s_max = 0u;
        s_nsplit = 0u;
        s_longest = 0u;
        s_total = 0ull;
    }
    __syncthreads();
    uint32_t m = 0u, ml = 0u;
    unsigned long long total = 0ull;
    const uint4 *cost4 = reinterpret_cast<const uint4 *>(cost);
#pragma unroll 4
    for (uint32_t i = tid; i < n; i += 1024u) {
        const uint4 w = cost4[i]; // the four waves of the tile, most recent frame
        uint32_t v = w.x + w.y + w.z + w.w;
        uint32_t longest = max(max(w.x, w.y), max(w.z, w.w));
        const uint32_t was_split = extra ? (state[i] & 1u) : 0u;
        if (was_split) {
            const uint4 w2 = cost4[n + i]; // the waves of the second half
            v += w2.x + w2.y + w2.z + w2.w;
            longest = max(longest, max(max(w2.x, w2.y), max(w2.z, w2.w)));
            longest += (longest >> 2) + (longest >> 5); // what the wave would take unsplit
        }
        // (the classes come from the mean of this measurement and the running value: a tile's cycles depend on what
        // runs beside it, i.e. on the order itself, and an order made from one frame's costs alone keeps changing)
        const uint32_t prev = snap[i];
        if (prev) v = (uint32_t)(((unsigned long long)prev + v) >> 1);
        snap[i] = v;
        // (kept in 31 bits, and the frame's longest wave is the longest of what is KEPT: the bars and the classes below compare it with
        // state[] — against the unclamped maximum the longest wave itself fell below 0.85 x the longest and into a class of its own
        // making, and the order was no function of snap[] and state[])
        longest = min(longest, 0x7FFFFFFFu);
        state[i] = (longest << 1) | was_split;
        m = max(m, v);
        ml = max(ml, longest);
        total += v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        m = max(m, (uint32_t)__shfl_down(m, off, 64));
        ml = max(ml, (uint32_t)__shfl_down(ml, off, 64));
        total += __shfl_down(total, off, 64);
    }
    if (lane == 0u) {
        atomicMax(&s_max, m);
        atomicMax(&s_longest, ml);
        atomicAdd(&s_total, total);
    }
    __syncthreads(); // (also orders the snap[] / state[] writes before the reads of other threads below)
    const uint32_t mx = s_max;
    if (mx == 0u) { // no measurement yet: keep the current order
        if (order != prev_order)
            for (uint32_t i = tid; i < 8u * row; i += 1024u) order[i] = prev_order[i];
        for (uint32_t i = tid; i < n; i += 1024u) state[i] &= 1u;
        return;
    }
    // A frame whose slowest wave is well below (0.6 x) the time the frame needs anyway (its wave-cycles spread over all
    // wave slots) keeps the plain reverse-raster order: there the launch order cannot shorten anything.  Otherwise: cost
    // classes, and which tiles to split.
    const unsigned long long par = s_total / (wave_slots ? wave_slots : 1u);
    const bool reorder = (unsigned long long)s_longest * 5ull > par * 3ull;
    const unsigned long long threshold = par + (par >> 2);
    const uint32_t top_bar = (uint32_t)(0.85f * (float)s_longest); // (0.7: the headline's V1 +3 %; none: V1 / V2 +2 %)
#pragma unroll 4
    for (uint32_t i = tid; i < n; i += 1024u) {
        // (... and the frame's very longest waves whatever the bar says: a frame whose slowest wave is all of it — the headline's V1 / V2 —
        // ends with that wave)
        uint32_t want = (reorder && extra && ((unsigned long long)(state[i] >> 1) > threshold || (state[i] >> 1) > top_bar)) ? 1u : 0u;
        if (want && atomicAdd(&s_nsplit, 1u) >= extra) want = 0u; // no spare entry left
        state[i] = (state[i] & ~1u) | want; // (bits 1-31: the tile's slowest wave, for the class of a split tile below)
    }
    __syncthreads();
    const uint32_t nsplit = min(s_nsplit, extra);
    const float scale = reorder ? (float)kScheduleBuckets / (float)mx : 0.0f; // (0: one class, i.e. reverse raster)
    // ONE scale for all workgroups when tiles are split: the expected time of the workgroup's slowest wave — the tile's slowest wave,
    // over 1.28 for a half (what splitting gains) — so that a whole tile with a long wave is not launched behind every half
    const float split_scale = (float)kAllBuckets / (float)max(1u, s_longest);
    auto class_of = [&](uint32_t tile, uint32_t st) {
        if (nsplit != 0u) return min(kAllBuckets - 1u, (uint32_t)((float)(st >> 1) * ((st & 1u) ? 0.78125f : 1.0f) * split_scale));
        return min(kScheduleBuckets - 1u, (uint32_t)((float)snap[tile] * scale));
    };
    // thread t owns positions [lo, hi) of the default order (position j = tile n-1-j)
    const uint32_t chunk = (n + 1023u) / 1024u;
    const uint32_t lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    uint32_t cnt[kAllBuckets]; // classes kScheduleBuckets ...: the halves of split tiles
#pragma unroll
    for (uint32_t b = 0; b < kAllBuckets; b++) cnt[b] = 0u;
#pragma unroll 4
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t tile = n - 1u - j;
        const uint32_t st = state[tile], sp = st & 1u;
        const uint32_t b = class_of(tile, st);
#pragma unroll
        for (uint32_t k = 0; k < kAllBuckets; k++) cnt[k] += (k == b) ? (1u + sp) : 0u;
    }
    // exclusive scan of every class over the threads, heaviest class first: inside the wave by shuffles, over the 16 waves
    // by one thread per class
    uint32_t pos[kAllBuckets];
#pragma unroll
    for (uint32_t b = 0; b < kAllBuckets; b++) {
        uint32_t incl = cnt[b];
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= (uint32_t)off) incl += up;
        }
        pos[b] = incl - cnt[b]; // exclusive, inside the wave
        if (lane == 63u) wave_total[b][wv] = incl;
    }
    __syncthreads();
    if (tid < kAllBuckets) {
        uint32_t acc = 0u;
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t t = wave_total[tid][k];
            wave_total[tid][k] = acc; // -> exclusive over the waves
            acc += t;
        }
        class_total[tid] = acc;
    }
    __syncthreads();
    {
        uint32_t base = 0u;
#pragma unroll
        for (int b = (int)kAllBuckets - 1; b >= 0; b--) {
            pos[b] += base + wave_total[b][wv];
            base += class_total[b];
        }
    }
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t tile = n - 1u - j;
        const uint32_t st = state[tile], sp = st & 1u;
        const uint32_t b = class_of(tile, st);
        uint32_t at = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kAllBuckets; k++) {
            if (k == b) {
                at = pos[k];
                pos[k] += 1u + sp;
            }
        }
        if (sp) {
            order[(at & 7u) * row + (at >> 3)] = tile | 0x80000000u;
            order[((at + 1u) & 7u) * row + ((at + 1u) >> 3)] = tile | 0xC0000000u;
        } else {
            order[(at & 7u) * row + (at >> 3)] = tile;
        }
    }
    for (uint32_t at = n + nsplit + tid; at < 8u * row; at += 1024u) order[(at & 7u) * row + (at >> 3)] = 0xFFFFFFFFu; // idle workgroups
}
} // namespace vrt

namespace vrt_impl {
using vrt::ScheduleFrame;
using vrt::TileSchedule;
#define VRT_TRY(call) do { if (const hipError_t e_ = (call); e_ != hipSuccess) return e_; } while (0)

// one sort, on `stream`: the only place vrt_schedule_kernel is launched from.  cost: 8 n words; snap: 2 n (snapshot, split state); from / into: order
// buffers of 8 * ceil((n + extra_max) / 8) words (the same buffer: in place); extra, wave_slots: the rule (tiles it may split, its bar)
static hipError_t launch_schedule(hipStream_t stream, const uint32_t *cost, uint32_t *snap, const uint32_t *from, uint32_t *into, uint32_t n,
                                  uint32_t extra_max, uint32_t extra, uint32_t wave_slots) {
    VRT_LAUNCH(vrt::vrt_schedule_kernel, dim3(1), dim3(1024), 0, stream, cost, snap, from, into, n, extra_max, extra, wave_slots);
    return hipGetLastError();
}

// order `into` of the context sorted from its order `from` by the measured costs, on the primary stream; units, wave_slots: the rule
static hipError_t sort_orders(const vrt_ctx *ctx, uint32_t from, uint32_t into, uint32_t units, uint32_t wave_slots) {
    const TileSchedule &s = ctx->sched;
    uint32_t *const order = s.d_tile_schedule, *const snap = order + 2u * (size_t)s.stride;
    return launch_schedule(ctx->stream, s.d_tile_cost, snap, order + (size_t)from * s.stride, order + (size_t)into * s.stride, ctx->shard.owned_tiles, s.extra,
                           std::min(units, s.extra), wave_slots);
}

hipError_t schedule_create(vrt_ctx *c, uint32_t cus) {
    TileSchedule &s = c->sched;
    const uint32_t variant = c->cfg.kernel_variant;
    // tile schedule starts as reverse raster (bottom rows first); the feedback kernel refines it
    const uint32_t n = c->shard.owned_tiles ? c->shard.owned_tiles : 1u;
    // default order: frames that run one at a time take the amortised cost-feedback schedule (7) unless all their workgroups
    // are resident at once (6 per CU: no launch order to speak of) or the frame is many times that (4K: 21 rounds of resident
    // workgroups, the tail is a small part of it and the schedule measured +1 %); the schedule may split tiles (spare entries)
    uint32_t order = (variant >> 16) & 0xFu;
    s.order_auto = (order == 0u);
    if (order == 0u) order = (n > 6u * cus && n <= 64u * cus) ? 7u : 3u;
    s.tile_order = order;
    const bool plain_tiles = (vrt::resolve_variant(variant) & 0xFFu) != vrt::kVariantLinearLds512;
    // spare entries: one per tile (the list's layout); a sort may use min(1024, n / 8) of them — or all, with a lower bar, for
    // frames of two samples per pixel (measured on the reference app's run, same box, V0 / V1 / V2: 0.336 / 0.340 / 0.364 ms with
    // n / 8 and a bar of 1.25 x the frame's wave-cycles over 24 slots per CU; 0.294 / 0.306 / 0.330 with every tile eligible
    // and 40 slots per CU — 28 / 32 / 36 / 44: 0.329 / 0.306 / 0.293 / 0.295 on V0; every tile split 0.339 / 0.345 / 0.370; a cap
    // below what the bar asks for makes the order flip between sorts: n / 4 0.395 / 0.367 / 0.396)
    s.extra = (order == 7u && plain_tiles) ? n : 0u;
    s.cap[0] = std::min(std::min(1024u, n / 8u), s.extra), s.cap[1] = s.extra;
    s.slots[0] = 24u * cus; // 4 SIMDs x 6 waves of the trace kernel per CU
    // (with the halves in cost classes of their own — vrt_schedule_kernel, round 4 — a lower bar pays: 28 / 40 / 52 / 64 / 96 slots
    // per CU 0.300 / 0.260 / 0.259 / 0.259 / 0.259 ms on V0, 0.323 / 0.285 / 0.262 / 0.255 / 0.257 on V1, 0.350 / 0.312 / 0.286 / 0.284 / 0.282 on V2)
    s.slots[1] = 64u * cus;
    VRT_TRY(c->res.device(&s.d_tile_cost, n * 32u)); // [half][tile][wave]
    const uint32_t ns = s.stride = 8u * ((n + s.extra + 7u) / 8u); // an order buffer is stored XCD-major: 8 rows of ceil((n + extra) / 8)
    VRT_TRY(c->res.device(&s.d_tile_schedule, (2u * (size_t)ns + 2u * (size_t)n) * 4u)); // order A, order B, snapshot + split state
    VRT_TRY(hipMemsetAsync(s.d_tile_cost, 0, n * 32u, c->stream));
    VRT_TRY(hipMemsetAsync(s.d_tile_schedule + 2u * (size_t)ns, 0, 2u * (size_t)n * 4u, c->stream));
    std::vector<uint32_t> init(ns, 0xFFFFFFFFu); // spare entries: idle workgroups
    for (uint32_t i = 0; i < n; i++) init[(i & 7u) * (ns / 8u) + (i >> 3)] = n - 1u - i;
    VRT_TRY(hipMemcpy(s.d_tile_schedule, init.data(), ns * 4u, hipMemcpyHostToDevice));
    // first launch of the schedule kernel now (code-object load, about 2 ms, stays out of the frames): with no cost
    // measured yet it copies the initial order into the second buffer
    if (n > 1u) VRT_TRY(sort_orders(c, 0u, 1u, s.cap[0], s.slots[0]));
    if (order != 7u) return hipSuccess;
    // the cost-feedback schedule, re-sorted every 32 frames instead of every frame: the kernel sees order 5
    s.period = (variant >> 28) ? (1u << (variant >> 28)) : 32u; // tuning knob: log2 of the period
    VRT_TRY(c->res.event(&s.ev_sched, hipEventDisableTiming));
    return c->res.event(&s.ev_b_sched, hipEventDisableTiming);
}

void schedule_bind(const TileSchedule &s, vrt::TraceParams &p) {
    p.tile_order = s.tile_order == 7u ? 5u : s.tile_order, p.sched_extra = s.extra, p.sched_units = s.cap[0];
    p.tile_cost = s.d_tile_cost, p.tile_schedule = s.d_tile_schedule;
}

bool schedule_two_streams(const vrt_ctx *ctx) { return ctx->params.tile_order != 5u || ctx->sched.period; }

// which of the cost schedule's two rules serves this frame (vrt_trace_kernel's `dual`: two samples per pixel, whole RGBA pixels); a
// change re-sorts at once, on the primary stream (schedule_change_rule).  scheduled: the frame's kernel reads the schedule.
ScheduleFrame schedule_frame(const vrt_ctx *ctx, const vrt_camera_device *camera, bool scheduled) {
    const TileSchedule &s = ctx->sched;
    ScheduleFrame f{scheduled, false, false, (s.period && scheduled && camera->samples_per_pixel == 2 && !ctx->params.packed_rgb) ? 1u : 0u};
    f.changes = s.period && scheduled && f.rule != s.mode;
    // (frames of two samples per pixel keep the cost schedule on both streams: their split tiles trace the second sample on the idle
    // lanes, which is worth more than reverse raster's neighbourhood — the app's run, two frames in flight, V0 / V1 / V2: 0.205 /
    // 0.214 / 0.237 ms per frame against 0.267 / 0.262 / 0.286, tools/experiments/fif_order_ab.py)
    f.raster = s.order_auto && f.rule == 0u && !f.changes;
    return f;
}

hipError_t schedule_before_b(vrt_ctx *ctx) { // the schedule buffer this frame reads was sorted on the primary stream
    return ctx->sched.b_seen != ctx->sched.seq ? hipStreamWaitEvent(ctx->stream_b, ctx->sched.ev_sched, 0) : hipSuccess;
}

hipError_t schedule_after_b(vrt_ctx *ctx) {
    TileSchedule &s = ctx->sched;
    if (s.b_seen != s.seq) {
        // everything this stream read from the OTHER schedule buffer is finished once this event is
        VRT_TRY(hipEventRecord(s.ev_b_sched, ctx->stream_b));
        s.b_recorded = true, s.b_seen = s.seq;
    }
    s.since++;
    return hipSuccess;
}

hipError_t schedule_sort_in_place(vrt_ctx *ctx, const ScheduleFrame &f) {
    if (!(ctx->params.tile_order == 5u && ctx->shard.owned_tiles > 1u && !ctx->sched.period && f.scheduled)) return hipSuccess;
    // re-sort the tile list by last frame's measured cost (inside the timed region: it is per-frame work)
    return sort_orders(ctx, 0u, 0u, 0u, ctx->sched.slots[0]);
}

hipError_t schedule_change_rule(vrt_ctx *ctx, const ScheduleFrame &f) {
    if (!f.changes) return hipSuccess;
    // The re-sort below writes the schedule buffer no frame is SUPPOSED to read any more — ev_b_sched covers the second stream's
    // reads of it only from the first stream-b frame behind the previous sort on.  A change of rule may follow a sort at once
    // (samples per pixel 2 -> 1 -> 2 on consecutive frames): then a frame still running on the second stream may read the very
    // buffer this sort rewrites.  Let the primary stream wait for the second stream's last frame.
    if (ctx->stream_b && ctx->b_pending) {
        VRT_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_b_done, 0));
        ctx->b_pending = false;
    }
    ctx->sched.mode = f.rule, ctx->params.sched_units = ctx->sched.cap[f.rule];
    ctx->sched.since = ctx->sched.period; // (the sort is due: schedule_before_frame)
    return hipSuccess;
}

hipError_t schedule_before_frame(vrt_ctx *ctx, const ScheduleFrame &f) {
    TileSchedule &s = ctx->sched;
    if (s.period && ctx->shard.owned_tiles > 1u && s.since >= s.period && f.scheduled) {
        // Amortised re-sort, in the frames' own stream (inside the timed region as well): the measured costs (running mean)
        // order the tiles into the buffer no frame reads; frames launched from here on read that one.  A sort costs about
        // 35 us of the stream's time (the kernel plus the two kernel boundaries).  Measured alternatives: on a second
        // stream with event waits 80 us per sort; on a second stream with the host polling for its completion nothing, but
        // then the order lags behind frames that are queued ahead (vrt_dispatch_repeat) by a whole call.
        if (s.b_recorded) VRT_TRY(hipStreamWaitEvent(ctx->stream, s.ev_b_sched, 0)); // (signalled a period ago)
        VRT_TRY(sort_orders(ctx, s.cur, s.cur ^ 1u, s.cap[s.mode], s.slots[s.mode]));
        VRT_TRY(hipEventRecord(s.ev_sched, ctx->stream));
        s.cur ^= 1u;
        ctx->params.tile_schedule = s.d_tile_schedule + (size_t)s.cur * s.stride;
        s.seq++, s.since = 0;
    }
    s.since++;
    return hipSuccess;
}

// (the cost-ordered launch has spare workgroups for the halves of split tiles: any number up to the list's spare entries, by the rule)
uint32_t schedule_groups(const vrt_ctx *ctx, bool any_rule) {
    return ctx->shard.owned_tiles + (ctx->params.tile_order == 5u ? (any_rule ? ctx->sched.extra : ctx->params.sched_units) : 0u);
}
#undef VRT_TRY
} // namespace vrt_impl

using namespace vrt_impl;

extern "C" {

// ---- read-back and a sort on the caller's arrays: a test and diagnosis aid (include/vrt_hip.h) ----

int vrt_schedule_info(const vrt_ctx *ctx, uint32_t out[12]) {
    if (!ctx || !out) return VRT_E_INVALID_ARG;
    const vrt::TileSchedule &s = ctx->sched;
    const uint32_t v[12] = {s.tile_order, ctx->shard.owned_tiles, s.extra, s.stride, s.cur, s.mode, s.cap[0], s.cap[1], s.slots[0], s.slots[1], s.period, (uint32_t)s.seq};
    std::copy(v, v + 12, out);
    return VRT_OK;
}

int vrt_read_schedule(vrt_ctx *ctx, uint32_t part, void *dst, uint64_t nbytes) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (part >= VRT_SCHEDULE_PART_COUNT) return fail(ctx, VRT_E_INVALID_ARG, "bad schedule part");
    if (nbytes && !dst) return fail(ctx, VRT_E_INVALID_ARG, "dst is NULL");
    const vrt::TileSchedule &s = ctx->sched;
    if (!s.d_tile_schedule || !s.d_tile_cost) return fail(ctx, VRT_E_STATE, "this context holds no tile schedule");
    const size_t n = ctx->shard.owned_tiles ? ctx->shard.owned_tiles : 1u; // (what schedule_create sized the buffers for)
    const uint32_t *src = nullptr;
    size_t words = 0;
    switch (part) {
    case VRT_SCHEDULE_ORDER_CURRENT: src = s.d_tile_schedule + (size_t)s.cur * s.stride, words = s.stride; break;
    case VRT_SCHEDULE_ORDER_OTHER: src = s.d_tile_schedule + (size_t)(s.cur ^ 1u) * s.stride, words = s.stride; break;
    case VRT_SCHEDULE_SNAPSHOT: src = s.d_tile_schedule + 2u * (size_t)s.stride, words = n; break;
    case VRT_SCHEDULE_SPLIT_STATE: src = s.d_tile_schedule + 2u * (size_t)s.stride + n, words = n; break;
    default: src = s.d_tile_cost, words = 8u * n; break;
    }
    if (nbytes > words * 4u) return fail(ctx, VRT_E_OUT_OF_RANGE, "read exceeds the schedule part");
    if (nbytes == 0) return VRT_OK;
    DeviceGuard dg(ctx->device);
    VRT_HIP(ctx, wait_stream(ctx->stream)); // (frames and sorts of both streams write what is read here)
    if (ctx->stream_b) VRT_HIP(ctx, wait_stream(ctx->stream_b));
    VRT_HIP(ctx, hipMemcpy(dst, src, nbytes, hipMemcpyDeviceToHost));
    return VRT_OK;
}

int vrt_schedule_sort(vrt_ctx *ctx, const uint32_t *cost, uint32_t *snap_state, const uint32_t *prev_order, uint32_t *order, uint32_t n, uint32_t extra_max,
                      uint32_t extra, uint32_t wave_slots, uint32_t in_place) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (!cost || !snap_state || !prev_order || !order) return fail(ctx, VRT_E_INVALID_ARG, "a NULL array");
    if (n == 0u) return fail(ctx, VRT_E_INVALID_ARG, "n is 0");
    if (extra > extra_max) return fail(ctx, VRT_E_INVALID_ARG, "extra exceeds extra_max");
    if (n > (1u << 24) || extra_max > (1u << 24)) return fail(ctx, VRT_E_OUT_OF_RANGE, "more than 2^24 tiles or spare entries");
    // one allocation: guard | cost | guard | snapshot + state | guard | previous order | guard | order | guard (in place: one order buffer), each
    // buffer of exactly its documented size, so that a write one word outside lands in a guard
    constexpr size_t kGuard = 64; // words; keeps cost (read as uint4) 16-byte aligned
    constexpr uint32_t kGuardWord = 0x6A5D0000u, kFill = 0x5EED5EEDu;
    const size_t ns = 8u * (((size_t)n + extra_max + 7u) / 8u);
    const size_t at_cost = kGuard, at_snap = at_cost + 8u * (size_t)n + kGuard, at_prev = at_snap + 2u * (size_t)n + kGuard;
    const size_t at_order = in_place ? at_prev : at_prev + ns + kGuard, total = at_order + ns + kGuard;
    std::vector<uint32_t> host(total), back(total);
    for (size_t i = 0; i < total; i++) host[i] = kGuardWord | (uint32_t)(i & 0xFFFFu); // (every word that is no buffer is a guard)
    std::copy(cost, cost + 8u * (size_t)n, host.begin() + at_cost);
    std::copy(snap_state, snap_state + 2u * (size_t)n, host.begin() + at_snap);
    if (!in_place) std::fill(host.begin() + at_order, host.begin() + at_order + ns, kFill);
    std::copy(prev_order, prev_order + ns, host.begin() + at_prev);
    DeviceGuard dg(ctx->device);
    uint32_t *d = nullptr;
    if (const hipError_t e = hipMalloc(&d, total * 4u); e != hipSuccess) return hip_fail(ctx, e, "hipMalloc of the sort's scratch buffers");
    hipError_t e = hipMemcpy(d, host.data(), total * 4u, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_schedule(ctx->stream, d + at_cost, d + at_snap, d + at_prev, d + at_order, n, extra_max, extra, wave_slots);
    if (e == hipSuccess) e = wait_stream(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(back.data(), d, total * 4u, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(ctx, e, "vrt_schedule_sort");
    std::copy(back.begin() + at_snap, back.begin() + at_snap + 2u * (size_t)n, snap_state);
    std::copy(back.begin() + at_order, back.begin() + at_order + ns, order);
    const auto buffer = [&](size_t i) {
        return (i >= at_cost && i < at_cost + 8u * (size_t)n) || (i >= at_snap && i < at_snap + 2u * (size_t)n) || (i >= at_prev && i < at_prev + ns) ||
               (i >= at_order && i < at_order + ns);
    };
    for (size_t i = 0; i < total; i++)
        if (!buffer(i) && back[i] != host[i]) return fail(ctx, VRT_E_STATE, "vrt_schedule_kernel wrote outside its buffers (guard word " + std::to_string(i) + ")");
    for (size_t i = at_cost; i < at_cost + 8u * (size_t)n; i++)
        if (back[i] != host[i]) return fail(ctx, VRT_E_STATE, "vrt_schedule_kernel wrote to the costs");
    if (!in_place)
        for (size_t i = at_prev; i < at_prev + ns; i++)
            if (back[i] != host[i]) return fail(ctx, VRT_E_STATE, "vrt_schedule_kernel wrote to the previous order");
    return VRT_OK;
}

} // extern "C"
