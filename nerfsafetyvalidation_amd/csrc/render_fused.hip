// render_fused.hip -- the MI355X-native body of NeRFRenderer.run_cuda (eval branch,
// nerf/renderer.py:329-378): march -> hash-grid encode -> sigma MLP -> SH ->
// colour MLP -> composite -> stable compaction, one fused kernel per reference loop iteration.
//
// What the reference does per iteration (6+ launches, 3 zero-filled [M,*] tensors, a host sync
// for the boolean-mask compaction) becomes two launches and no host round trip:
//
//   k_render_iter   512-thread workgroups (8 waves).  A wave owns 64 alive rays:
//     1. lane = ray: occupancy-grid DDA (ngp::Dda; same sample sequence as march_rays, reached with the exact
//        shortcuts of Dda::probe_lin / skip_const_dt / jump_block, occupancy.hpp) emits up to kCh sample parameters (t, dt)
//        per sub-pass into the wave's LDS slab -- no [M,3] xyzs/dirs/deltas;
//     2. the wave's valid samples are compacted (wave prefix sum) and processed 16 at a time:
//        lane = (sample c = lane & 15, quarter q = lane >> 4).  Each lane gathers 4 of the 16
//        hash levels (q, q+4, q+8, q+12; 32 four-byte table reads in flight per lane) and
//        interpolates them (fp32 accumulation, one rounding to fp16).  Its 8 features ARE the
//        B fragment of v_mfma_f32_16x16x32_f16 for the TRANSPOSED product H^T = W * X^T, so
//        the encoder output never touches memory.  Every following layer consumes the previous
//        accumulator directly as its B fragment (the k-order permutation this implies is folded
//        into the weight fragments once, by k_pack_weights); activations never leave registers.
//        Weights live in LDS as ready-made A fragments (16 B per lane, conflict-free b128 reads).
//     3. lane = ray again: composite_rays arithmetic on the wave's LDS results, state update,
//        survivor ballot -> block-local stable compaction into a staging list.
//   k_render_compact  stitches the per-group survivor lists into the next alive list (stable; rays whose next
//        march starts in empty space first) and evaluates the reference's schedule on the device:
//        n_step = clamp(N // n_alive, 1, 8), step += n_step, stop when step >= max_steps.
//
// The host enqueues iterations ahead of the device-side state (kernels read n_alive / n_step from
// device memory and return immediately once `done` is set) and learns the state through a pinned
// status ring, so the stream never drains while the host catches up.
//
// Numerics: the operator kernels' expressions (explicit fmaf, -ffp-contract=off) except the fp32 corner accumulation
// noted above; DESIGN.md section 5.
//
// The network itself (NetArgs, stage_block, net_density / net_color) is fused_net.hpp; the uniform-sample renderer, the point
// queries and weight packing are units of their own (DESIGN.md "Fused sources").
#include <hip/hip_fp16.h>
#include <math.h>
#include <string.h>

#include <atomic>

#include "fused_net.hpp"
#include "launch_plan.hpp"
#include "occupancy.hpp"

namespace ngp {

constexpr int kWaves = 8;                 // waves per workgroup
constexpr int kThreads = kWaves * 64;     // 512
constexpr int kWavesPerSimd = 4;          // two 512-thread workgroups per CU (LDS: 2 x ~72 KB)
constexpr int kCh = 2;                    // march steps handled per sub-pass (n_step <= 8 is processed in chunks of kCh)
constexpr int kSlots = 64 * kCh;          // sample slots per wave and sub-pass
constexpr size_t kLinMaxBytes = 4u << 20;  // linear copy of the occupancy bitfield (C * H^3 / 8 bytes)
constexpr int kLookahead = 4;             // iterations the host may enqueue beyond the last status it has seen
constexpr int kRing = 8;

// The loop state (struct Ctl), the schedule of "several reference iterations per launch" and every transition of it are
// launch_plan.hpp's: one integer state machine, host and device, which tests/test_launch_plan_cpu.py runs whole on the CPU.
constexpr int kDeathShards = 64;
// per launch parity: [kDeathShards][kSpecK] deaths per iteration (k_render_iter) | [kDeathShards][kSpecK] rays whose MARCH runs out of
// samples in that iteration (k_march_ahead: known before the network runs, see truncate_launch) | [kDeathShards][kForecastBuckets]
// the saturation forecast of the launch's survivors (k_render_iter step 4 -> the sizing code of k_render_compact, nothing else).
// The first two blocks are cleared right before a multi-iteration launch uses them, the forecast before EVERY launch -- always the
// other parity's, never the buffer the running k_render_compact's blocks are reading (DESIGN "A race found by sharing the GPU").
constexpr uint32_t kForecastAt = 2u * kDeathShards * kSpecK;
constexpr uint32_t kDeathWords = kForecastAt + kDeathShards * kForecastBuckets;
// work-queue heads: one per shard (chunk c belongs to shard c & 7), each on its own 128-byte line, two sets (ping-pong with Ctl)
struct QueueHeads { uint32_t head[8][32]; };

constexpr int kStatShards = 64;   // sample counters are sharded: a single hot atomic serialises at ~90 ops/us chip-wide

// ------------------------------------------------------------------------------------------
// render iteration
// ------------------------------------------------------------------------------------------
struct RenderArgs {
    const float *rays_o, *rays_d, *fars;
    float* rays_t;
    float *weights_sum, *depth, *image;
    float *last_sigmas, *last_rgbs;   // optional dump of the iteration's slot-major outputs
    float pad_sigma, pad_r, pad_g, pad_b;
    float4* dump_rec;                 // [N][8] per-RAY records (sigma, r, g, b) of the current iteration, used instead of the slot-major rows
    uint32_t* dump_iter;              // [N]    when the alive list is regrouped (sort_slow): k_dump_gather restores the reference's row order
    const int32_t* alive_in;
    int32_t* staging;                 // [chunks*64] chunk-local compacted survivors
    uint32_t* chunk_count;            // [chunks] survivors per chunk: fast | slow << 16 (see sort_slow)
    uint32_t sort_slow;               // group survivors whose next march starts in empty space at the END of the next alive list
    Ctl* ctl;                         // state read by this iteration
    QueueHeads* heads;                // its work-queue heads (zeroed by the previous k_render_compact / k_render_init)
    unsigned long long* stat_shards;  // [kStatShards] marched-sample counters (summed by k_render_compact)
    uint32_t* death_shards;           // [kDeathShards][kSpecK] rays that died in the k-th iteration of a speculative launch
    float4* backup;                   // [N][2] per-ray state before a speculative launch (restored if its verification fails)
    const uint8_t* bitfield;
    uint32_t cascade, grid_size, max_steps, perturb;
    float dt_gamma;
    Pcg32 rng;
    // coarse occupancy bits, staged into LDS (coarse_words == 0: unfiltered probes).  LIN kernels: with the x-fastest copy of the bitfield
    // and log2(grid_size), both in x-fastest order; otherwise `coarse` alone, in the bitfield's Morton order (k_build_coarse)
    OccupancyLin occ;
    uint32_t block_jump;              // LIN kernels: leave empty 4x4x4 blocks in one step (Dda::jump_block)
    uint32_t* sample_hash;            // diagnostics (ngp_debug_set_sample_hash): per-ray FNV hash of the marched (dt, delta1) bit patterns
    unsigned long long* stamps;       // diagnostics only (ngp_debug_set_stamps): per-phase cycle sums; NULL in normal runs
    // what k_march_ahead leaves for k_render_iter: the (t, dt) of every sample of this launch, [chunk][sample][lane] (a wave's 64 rays of one
    // sample index are 512 contiguous bytes), and per list entry the number of samples marched (bits 0-5) + the slow-ray flag (bit 7)
    float2* march_samples;
    uint8_t* march_counts;
    uint32_t wave_slots;              // waves the chip holds for this launch (item_width)
    uint32_t n_rays;                  // N: the reference's n_step = clamp(N // n_alive, 1, 8)
    uint32_t pre_verdict;             // k_march_ahead counts the rays whose march runs out per iteration (truncate_launch); 0: diagnostics
    uint32_t wave_march_max;          // launches of at most this many rays march one WAVE per ray (march_ahead_wave); 0: never
    uint32_t cell_runs;               // k_march_ahead: the samples that follow a probe's in the same occupied cell are taken without probing
    uint32_t forecast;                // k_render_iter leaves the saturation forecast of its survivors (death_shards + kForecastAt); 0: diagnostics
};

// Work items of k_render_iter: W consecutive entries of the alive list, one wave each.  64 while the list fills the chip's wave slots
// (every lane of the per-ray phases busy); 32 / 16 once it no longer does -- the late iterations of a frame, and most of a frame whose
// rays mostly miss the scene (BASELINE configs[3]: cameras outside the box): a launch then lasts as long as ONE item's sub-passes, and
// narrower items spread the same tiles over four times the waves.  The tile phases are 16 samples wide either way.  Both kernels of
// a launch derive W from the launch's n_alive.
__host__ __device__ __forceinline__ uint32_t item_width(uint32_t n_alive, uint32_t wave_slots) {
    return n_alive >= 64u * wave_slots ? 64u : (n_alive >= 32u * wave_slots ? 32u : 16u);
}
// an upper bound of the items of a launch whose n_alive is at most `ub`
static uint32_t items_bound(uint32_t ub, uint32_t wave_slots) {
    const uint32_t by64 = div_up(ub ? ub : 1, 64), narrow = div_up(ub ? ub : 1, 16);
    const uint32_t cap = 2u * wave_slots + 1u;                 // W < 64 only below 64 * wave_slots entries: at most this many items
    return by64 > (narrow < cap ? narrow : cap) ? by64 : (narrow < cap ? narrow : cap);
}

struct WaveSlab {  // per-wave LDS: kCh march steps of 64 rays
    float t[kSlots], dt[kSlots], sig[kSlots];
    uint32_t rg[kSlots], b[kSlots];
    uint16_t list[kSlots];
    float od[64][6];
};

// one row of the reference's last-iteration tensors (renderer.py:383-384): slot-major row (alive list in reference order) or,
// when the alive list is regrouped, a per-ray record that k_dump_gather sorts back into reference order after the loop
__device__ __forceinline__ void dump_row(const RenderArgs& ra, uint32_t entry, int32_t ray, uint32_t n_step, uint32_t k, float sg, float r,
                                         float g, float b) {
    if (ra.dump_rec) {
        ra.dump_rec[(size_t)ray * 8 + k] = make_float4(sg, r, g, b);
    } else {
        const size_t row = (size_t)entry * n_step + k;
        ra.last_sigmas[row] = sg;
        ra.last_rgbs[row * 3] = r; ra.last_rgbs[row * 3 + 1] = g; ra.last_rgbs[row * 3 + 2] = b;
    }
}

// ------------------------------------------------------------------------------------------
// The occupancy-grid march of one launch, on its own (raymarching.cu:757-813 for every live ray, all of the launch's samples).
// It used to run inside k_render_iter's waves, lane = ray, in lock-step: a third of the wave time at a lane utilisation of 0.44, in
// waves that hold the MLPs' 128 registers (4 per SIMD).  A ray's sample sequence does not depend on the network -- only on where
// compositing stops it -- so the march of ALL samples a launch may need is taken out: one lane per ray in small, register-light
// waves (full occupancy hides the probe latency chain), results through a [chunk][sample][lane] buffer that the network waves read
// back as whole lines.  Samples of rays that stop early are marched for nothing (the reference marches them too: march_rays runs
// n_step samples for every alive ray before composite_rays looks at any).  The sequence is the one k_render_iter produced: same
// Dda, same restart of the march at the iteration boundaries of a multi-iteration launch (from the re-accumulated rays_t), same jitter.
// LIN: power-of-two grid with the linear copies of the occupancy bits (Dda::probe_lin); otherwise the Morton-order originals
// ------------------------------------------------------------------------------------------
// The same march with one WAVE per ray, for the launches of a frame's tail: a few thousand rays, up to 32 samples each -- a lane per ray
// leaves the chip empty and the launch lasts as long as one ray's chain of dependent probes (60-80 us).  With a constant step
// (dt_gamma == 0) the lanes probe the 64 lattice points of a window at once and the wave follows the march's chain through them from
// registers, collecting the samples it visits (probe_window, occupancy.hpp, where the argument for its exactness is written); windows
// also end at the iteration boundaries inside the launch.  Same samples, same (t, dt) bits, same deltas -- k_render_iter cannot tell
// the two forms apart.
__device__ __forceinline__ void march_ahead_wave(const RenderArgs& ra, float bound, const Ctl& ctl, const uint32_t* coarse) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t entry = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (entry >= ctl.n_alive) return;
    const uint32_t n_step = ctl.n_step, spec = ctl.spec;
    const int32_t ray = ra.alive_in[entry];
    Dda dda;
    const float t_c = ra.rays_t[ray], far = ra.fars[ray];
    float t_march = dda.start(ra.rays_o + (size_t)ray * 3, ra.rays_d + (size_t)ray * 3, ra.bitfield, bound, 0.0f, ra.max_steps, ra.cascade,
                              ra.grid_size, &ra.occ, ra.block_jump != 0, t_c, ra.perturb, ra.rng, entry);
    float last_m = t_march, geo_tc = t_c;
    uint32_t emitted = 0, rounds = 0;
    float2* out = ra.march_samples + ((size_t)(entry >> 6) * n_step) * 64 + (entry & 63u);
    while (t_march < far && emitted < n_step) {
        rounds++;
        const LatticeWindow w = probe_window(dda, t_march, far, lane, coarse);
        // samples until the iteration boundary inside the launch (march_rays starts again from rays_t there), or the end of the launch
        const uint32_t room = spec ? spec - emitted % spec : n_step - emitted;
        unsigned long long emit = 0ull;
        uint32_t cur = 0, cnt = 0;
        float t_next = t_march;
        for (int guard = 0; guard < 64; guard++) {             // (the chain is strictly increasing: at most 64 points)
            const float to = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(w.nxt), (int)cur));
            if ((w.omask >> cur) & 1ull) {
                emit |= 1ull << cur;
                const float d1 = to - last_m;                  // deltas[1] of this sample (:791-793)
                last_m = to;
                geo_tc += d1;
                if (++cnt == room) { t_next = to; break; }
            }
            const uint32_t jn = (uint32_t)__builtin_amdgcn_readlane((int)w.j, (int)cur);
            if (jn >= 64u || !((w.vmask >> jn) & 1ull)) { t_next = to; break; }
            cur = jn;
        }
        if ((emit >> lane) & 1ull) out[(size_t)(emitted + (uint32_t)__popcll(emit & ((1ull << lane) - 1ull))) * 64] = make_float2(w.p, w.dt);
        emitted += cnt;
        t_march = t_next;
        if (spec && cnt == room) {                             // iteration boundary: from the re-accumulated rays_t, with last_t = t
            t_march = geo_tc;
            last_m = geo_tc;
        }
    }
    if (lane != 0) return;
    if (ra.stamps) {   // diagnostics: a window counts as one probe of the ray
        atomicAdd(ra.stamps + 4, (unsigned long long)rounds);
        atomicAdd(ra.stamps + 5, (unsigned long long)rounds * 64ull);
        atomicAdd(ra.stamps + 6, 1ull);
        atomicMax(ra.stamps + 7, (unsigned long long)rounds);
    }
    if (spec && ra.pre_verdict && emitted < n_step)
        atomicAdd(ra.death_shards + (size_t)kDeathShards * kSpecK + (blockIdx.x % kDeathShards) * kSpecK + emitted / spec, 1u);
    bool slow = false;
    if (ra.sort_slow && emitted == n_step) slow = geo_tc < far && dda.coarse_empty_at_lin(geo_tc, coarse);
    ra.march_counts[entry] = (uint8_t)(emitted | (slow ? 128u : 0u));
}

template <bool LIN>
__global__ void __launch_bounds__(256) k_march_ahead(RenderArgs ra, float bound) {
    const Ctl ctl = *ra.ctl;
    if (ctl.done) return;
    const uint32_t n_alive = ctl.n_alive, n_step = ctl.n_step, spec = ctl.spec;
    const bool by_wave = LIN && n_alive <= ra.wave_march_max;
    if (blockIdx.x * (by_wave ? 4u : 256u) >= n_alive) return;
    __shared__ uint32_t coarse_lds[kCoarseMaxBytes / 4];
    stage_coarse(ra.occ, coarse_lds, blockDim.x);
    __syncthreads();
    const uint32_t* coarse = ra.occ.coarse_words ? coarse_lds : nullptr;
    if (LIN && by_wave) {
        march_ahead_wave(ra, bound, ctl, coarse);
        return;
    }
    const uint32_t entry = blockIdx.x * blockDim.x + threadIdx.x;
    if (entry >= n_alive) return;
    const int32_t ray = ra.alive_in[entry];
    Dda dda;
    const float t_c = ra.rays_t[ray], far = ra.fars[ray];
    float t_march = dda.start(ra.rays_o + (size_t)ray * 3, ra.rays_d + (size_t)ray * 3, ra.bitfield, bound, ra.dt_gamma, ra.max_steps, ra.cascade,
                              ra.grid_size, LIN ? &ra.occ : nullptr, ra.block_jump != 0, t_c, ra.perturb, ra.rng, entry);
    float last_m = t_march;              // the march's last_t (:727-731)
    float geo_tc = t_c;                  // rays_t as composite_rays re-accumulates it (:848): where the next iteration's march restarts
    uint32_t emitted = 0;
    float2* out = ra.march_samples + ((size_t)(entry >> 6) * n_step) * 64 + (entry & 63u);
    float x, y, z, dt;
    uint32_t probes = 0, probes_coarse_empty = 0, probes_fine_empty = 0;   // diagnostics (ra.stamps): probes of this lane
    const bool run_cells = LIN && dda.const_dt && ra.cell_runs != 0;
    float occ_until = 0.0f;              // see Dda::probe_lin: positions before it lie in the occupied cell of the last probe
    while (t_march < far && emitted < n_step) {
        probes++;
        const bool diag_ce = LIN && ra.stamps && dda.coarse_empty_at_lin(t_march, coarse);
        const uint32_t emitted_before = emitted;
        if (LIN ? dda.probe_lin(t_march, x, y, z, dt, coarse, run_cells ? &occ_until : nullptr) : dda.probe(t_march, x, y, z, dt, coarse)) {
            // the sample of the probe, then the samples that follow in the same cell: no probe needed to know they are samples
            do {
                out[(size_t)emitted * 64] = make_float2(t_march, dt);
                t_march += dt;
                const float d1 = t_march - last_m;   // deltas[1] of this sample (:791-793)
                last_m = t_march;
                geo_tc += d1;
                emitted++;
                if (spec && emitted % spec == 0) {   // iteration boundary inside the launch: march_rays starts again from rays_t with last_t = t
                    t_march = geo_tc;
                    last_m = geo_tc;
                }
            } while (run_cells && t_march < occ_until && t_march < far && emitted < n_step);
        }
        if (ra.stamps && emitted == emitted_before) { if (diag_ce) probes_coarse_empty++; else probes_fine_empty++; }
    }
    // Rays whose next march begins inside an empty 4x4x4 block are about to skip through empty space (tens of DDA probes) while the
    // others take one probe per sample: k_render_iter groups them into their own chunks (a scheduling decision only).  The flag is
    // meaningful for rays that complete all n_step samples -- the survivors -- whose rays_t then is geo_tc.
    if (ra.stamps) {   // diagnostics only: [4] sum over waves of the slowest lane's probes, [5] all probes, [6] waves, [7] the slowest lane of all
        uint32_t mx = probes, sm = probes;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)mx, off, 64), p2 = (uint32_t)__shfl_xor((int)sm, off, 64);
            mx = mx > o ? mx : o;
            sm += p2;
        }
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__ballot(true))) {
            atomicAdd(ra.stamps + 4, (unsigned long long)mx);
            atomicAdd(ra.stamps + 5, (unsigned long long)sm);
            atomicAdd(ra.stamps + 6, 1ull);
            atomicMax(ra.stamps + 7, (unsigned long long)mx);
        }
        // [14] probes that found their 4x4x4 block empty, [15] probes in an occupied block that found their cell empty
        uint32_t ce = probes_coarse_empty, fe = probes_fine_empty;
        ce = wave_sum(ce);
        fe = wave_sum(fe);
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__ballot(true))) {
            atomicAdd(ra.stamps + 14, (unsigned long long)ce);
            atomicAdd(ra.stamps + 15, (unsigned long long)fe);
        }
    }
    if (spec && ra.pre_verdict) {     // the iteration of this launch in which the ray's march runs out (truncate_launch); wave-aggregated, sharded counters
        const uint32_t K = n_step / spec, jd = emitted < n_step ? emitted / spec : 0xFFFFFFFFu;
        const unsigned long long act = __ballot(true);
        const bool leader = (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(act);
        uint32_t* ex = ra.death_shards + (size_t)kDeathShards * kSpecK + (blockIdx.x % kDeathShards) * kSpecK;
        for (uint32_t j = 0; j < K; j++) {
            const unsigned long long b = __ballot(jd == j);
            if (leader && b) atomicAdd(&ex[j], (uint32_t)__popcll(b));
        }
    }
    bool slow = false;
    if (ra.sort_slow && emitted == n_step) slow = geo_tc < far && (LIN ? dda.coarse_empty_at_lin(geo_tc, coarse) : dda.coarse_empty_at(geo_tc, coarse));
    ra.march_counts[entry] = (uint8_t)(emitted | (slow ? 128u : 0u));
}

// CLAMPED: the positions below are clamped to [-bound, bound] and the host found 2*bound a power of two, so the encoder's
// out-of-range test cannot fire and is not compiled (encoder_unit in fused_net.hpp)
template <int MODE, bool HACC = false, bool CLAMPED = false>
__global__ void __launch_bounds__(kThreads, kWavesPerSimd) k_render_iter(NetArgs na, GridLevels lv, RenderArgs ra) {
    Ctl ctl = *ra.ctl;
    if (ctl.done) return;
    const uint32_t n_step_marched = ctl.n_step;     // k_march_ahead's buffer is laid out for the launch as it was planned
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (ctl.spec) {
        // (in the dynamic allocation, which is sized up to the CU's whole LDS: the weights' place, before stage_block fills it)
        uint32_t* exhausted = reinterpret_cast<uint32_t*>(smem);
        if (threadIdx.x < kSpecK) {
            uint32_t d = 0;
            for (int sh = 0; sh < kDeathShards; sh++) d += ra.death_shards[(size_t)kDeathShards * kSpecK + sh * kSpecK + threadIdx.x];
            exhausted[threadIdx.x] = d;
        }
        __syncthreads();
        truncate_launch(ctl, exhausted, ra.n_rays);
        __syncthreads();
    }
    const uint32_t n_alive = ctl.n_alive, n_step = ctl.n_step;
    const uint32_t spec = ctl.spec;    // != 0: the launch covers n_step / spec reference iterations of `spec` samples each (see Ctl)
    const uint32_t W = item_width(n_alive, ra.wave_slots);
    const uint32_t n_chunks = (n_alive + W - 1) / W;        // work items (see item_width)

    const size_t w_bytes = net_w_bytes_f16(na);
    _Float16* Wlds = reinterpret_cast<_Float16*>(smem);
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + w_bytes);
    WaveSlab* slabs = reinterpret_cast<WaveSlab*>(smem + w_bytes + sizeof(LevelTab));
    stage_block(na, lv, Wlds, lt, w_bytes);   // the only workgroup barrier: waves are independent from here on

    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, c = lane & 15;
    WaveSlab& S = slabs[wid];
    unsigned long long ts0 = 0, ts1 = 0;
#define NGP_STAMP(idx)                                                                  \
    if (ra.stamps) {                                                                    \
        ts1 = __builtin_amdgcn_s_memtime();                                             \
        if (lane == 0) atomicAdd(ra.stamps + (idx), ts1 - ts0);                         \
        ts0 = ts1;                                                                      \
    }

    // every wave pulls 64-ray chunks from a device-side queue: no inter-wave coupling, no tail imbalance.  The queue is
    // sharded up to 8 ways (chunk c lives in shard c % n_shards, heads on separate cache lines; a single hot atomic serialises at ~90
    // ops/us chip-wide); a workgroup serves the shard of its XCD group.  Shards hold equal work, so there is no stealing.
    const uint32_t n_shards = gridDim.x < 8u ? gridDim.x : 8u;   // every shard must have a workgroup serving it
    const uint32_t shard = blockIdx.x % n_shards;
    unsigned long long wave_total = 0;
    for (;;) {
        uint32_t chunk = 0xFFFFFFFFu;
        {
            uint32_t k = 0;
            if (lane == 0) k = atomicAdd(&ra.heads->head[shard][0], 1u);
            k = __builtin_amdgcn_readfirstlane(k);
            const uint32_t cand = k * n_shards + shard;
            if (cand < n_chunks) chunk = cand;
        }
        if (chunk == 0xFFFFFFFFu) break;
        if (ra.stamps) ts0 = __builtin_amdgcn_s_memtime();

        // the item's W entries keep their lanes of the 64-entry group they belong to (k_march_ahead's layout): lanes outside are idle
        const uint32_t first_entry = chunk * W, group = first_entry >> 6;
        const uint32_t entry = group * 64 + lane;
        const bool active = entry < n_alive && entry - first_entry < W;
        const int32_t ray = active ? ra.alive_in[entry] : -1;

        float last_t = 0, t_c = 0, t_c0 = 0, t_start = 0;
        float ws = 0, dep = 0, cr = 0, cg = 0, cb = 0;
        uint32_t emitted = 0;                // samples k_march_ahead marched for this lane's ray in this launch
        bool slow_next = false;              // ... and whether the ray's next march starts in an empty 4x4x4 block (if it survives)
        if (active) {
            t_c = ra.rays_t[ray];      // composite_rays' t (:848) accumulates from the unperturbed value
            t_c0 = t_c;
            t_start = t_c;
            if (ra.perturb) {          // where the march started: the first sample's deltas[1] counts from here (:727-731)
                const float SQRT3 = 1.7320508075688772f;
                Pcg32 rng = ra.rng;
                rng.advance((int64_t)entry);
                t_start += (2 * SQRT3 / (float)ra.max_steps) * rng.next_float();
            }
            last_t = t_start;
            const uint32_t mc = ra.march_counts[entry];
            emitted = mc & 63u;
            slow_next = (mc & 128u) != 0;
            ws = ra.weights_sum[ray]; dep = ra.depth[ray];
            cr = ra.image[(size_t)ray * 3]; cg = ra.image[(size_t)ray * 3 + 1]; cb = ra.image[(size_t)ray * 3 + 2];
#pragma unroll
            for (int d = 0; d < 3; d++) { S.od[lane][d] = ra.rays_o[(size_t)ray * 3 + d]; S.od[lane][3 + d] = ra.rays_d[(size_t)ray * 3 + d]; }
            if (spec) {   // the state this launch starts from, should its verification fail (k_render_compact restores it)
                ra.backup[(size_t)ray * 2] = make_float4(t_c, ws, dep, ra.sample_hash ? __uint_as_float(ra.sample_hash[ray]) : 0.0f);
                ra.backup[(size_t)ray * 2 + 1] = make_float4(cr, cg, cb, 0.0f);
            }
        }
        const float2* marched = ra.march_samples + ((size_t)group * n_step_marched) * 64 + lane;
        // ray states: running -> (terminated by T < 1e-4 | exhausted: the march ran out of samples) -> dead
        bool running = active;
        uint32_t steps_done = 0;      // samples composited so far (== n_step at the end <=> the ray survives)
        uint32_t wave_samples = 0;

        for (uint32_t s0 = 0; s0 < n_step; s0 += kCh) {
            const uint32_t want = (n_step - s0) < (uint32_t)kCh ? (n_step - s0) : (uint32_t)kCh;
            // ---- 1. march (raymarching.cu:757-813), lane = ray.  A ray whose compositing already stopped is not marched
            //         further unless the caller asked for the reference's last-iteration tensors.
            uint32_t cnt = 0;
            // (a launch that covers several iterations is never the reference's last one: nothing of it is dumped)
            const bool do_march = active && (running || (ra.last_sigmas != nullptr && !spec));
            if (do_march) {      // this sub-pass's samples, as k_march_ahead left them
                const uint32_t left = emitted > s0 ? emitted - s0 : 0u;
                cnt = left < want ? left : want;
                for (uint32_t k = 0; k < cnt; k++) {
                    const float2 v = marched[(size_t)(s0 + k) * 64];
                    S.t[lane * kCh + k] = v.x;
                    S.dt[lane * kCh + k] = v.y;
                }
            }
            if (!__any(cnt != 0)) {
                // nothing to evaluate in this sub-pass for the whole wave
                if (running && cnt < want) running = false;
                if (ra.last_sigmas && active && !spec)
                    for (uint32_t k = 0; k < want; k++) dump_row(ra, entry, ray, n_step, s0 + k, ra.pad_sigma, ra.pad_r, ra.pad_g, ra.pad_b);
                if (!ra.last_sigmas && !__any(running)) break;
                continue;
            }
            NGP_STAMP(0)
            // ---- 2. compact the wave's samples and run the network 16 at a time
            uint32_t incl = cnt;      // (wave_ops.hpp's scan_inclusive<AddOp> and last_lane, written out since the refactor that compared ISA)
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = __shfl_up(incl, off, 64);
                if (lane >= (uint32_t)off) incl += o;
            }
            const uint32_t total = __shfl(incl, 63, 64);
            for (uint32_t k = 0; k < cnt; k++) S.list[incl - cnt + k] = (uint16_t)((lane << 3) | k);
            const uint32_t n_tiles = (total + 15) / 16;
            unsigned long long sub_a = 0, sub_b = 0, sub_n = 0, sub_f = 0;   // diagnostics only
            uint32_t pre[8] = {0, 0, 0, 0, 0, 0, 0, 0};                      // MODE 2: the lane's hashed-level entries, gathered a tile ahead
            for (uint32_t tile = 0; tile < n_tiles; tile++) {
                const uint32_t j = tile * 16 + c;
                const bool valid = j < total;
                const uint32_t e = S.list[valid ? j : total - 1];
                const uint32_t rl = e >> 3, slot = rl * kCh + (e & 7);
                const float t = S.t[slot];
                const float ox = S.od[rl][0], oy = S.od[rl][1], oz = S.od[rl][2];
                const float dx = S.od[rl][3], dy = S.od[rl][4], dz = S.od[rl][5];
                const float x = clampf(fmaf(t, dx, ox), -na.bound, na.bound);
                const float y = clampf(fmaf(t, dy, oy), -na.bound, na.bound);
                const float z = clampf(fmaf(t, dz, oz), -na.bound, na.bound);
                float sg, r, g, b;
                if (ra.stamps) {   // diagnostics: split the tile into encode+sigma net and colour net, count tile fill
                    const unsigned long long ta = __builtin_amdgcn_s_memtime();
                    _Float16 s16[4];
                    net_density<MODE, HACC, CLAMPED>(na, Wlds, *lt, lane, x, y, z, sg, s16);
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    const unsigned long long tb = __builtin_amdgcn_s_memtime();
                    net_color(na, Wlds, lane, dx, dy, dz, s16, r, g, b);
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    const unsigned long long tc = __builtin_amdgcn_s_memtime();
                    sub_a += tb - ta;
                    sub_b += tc - tb;
                    sub_n += 1;
                    sub_f += min(16u, total - tile * 16);
                } else if (MODE == 2) {
                    // the hashed level is gathered one tile ahead (net_density_piped): position of the next tile's sample of this lane
                    const uint32_t jn = (tile + 1) * 16 + c;
                    const uint32_t en = S.list[jn < total ? jn : total - 1];      // (past the last tile: a valid entry, loaded for nothing)
                    const uint32_t rn = en >> 3;
                    const float tn = S.t[rn * kCh + (en & 7)];
                    const float nx = clampf(fmaf(tn, S.od[rn][3], S.od[rn][0]), -na.bound, na.bound);
                    const float ny = clampf(fmaf(tn, S.od[rn][4], S.od[rn][1]), -na.bound, na.bound);
                    const float nz = clampf(fmaf(tn, S.od[rn][5], S.od[rn][2]), -na.bound, na.bound);
                    if (tile == 0) hashed_gather<CLAMPED>(na, *lt, (lane >> 4) + 12, x, y, z, pre);
                    _Float16 s16[4];
                    net_density_piped<HACC, CLAMPED>(na, Wlds, *lt, lane, x, y, z, nx, ny, nz, pre, sg, s16);
                    net_color(na, Wlds, lane, dx, dy, dz, s16, r, g, b);
                } else {
                    _Float16 s16[4];
                    net_density<MODE, HACC, CLAMPED>(na, Wlds, *lt, lane, x, y, z, sg, s16);
                    net_color(na, Wlds, lane, dx, dy, dz, s16, r, g, b);
                }
                if (lane < 16 && valid) {
                    S.sig[slot] = na.density_scale * sg;   // renderer.py:365
                    S.rg[slot] = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)r) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)g) << 16);
                    S.b[slot] = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b);
                }
            }
            if (ra.stamps && lane == 0) {
                atomicAdd(ra.stamps + 8, sub_a); atomicAdd(ra.stamps + 9, sub_b); atomicAdd(ra.stamps + 10, sub_n); atomicAdd(ra.stamps + 11, sub_f);
            }
            NGP_STAMP(1)
            // ---- 3. composite (raymarching.cu:860-897), lane = ray
            if (running) {
                uint32_t k = 0;
                for (; k < cnt; k++) {
                    const uint32_t slot = lane * kCh + k;
                    const float dt = S.dt[slot];
                    const float t_after = S.t[slot] + dt;
                    const float delta1 = t_after - last_t;   // deltas[1] as march_rays wrote it (:791-793)
                    last_t = t_after;
                    const float sg = S.sig[slot];
                    const uint32_t rg = S.rg[slot];
                    const float sr = (float)__builtin_bit_cast(_Float16, (uint16_t)(rg & 0xffffu));
                    const float sgc = (float)__builtin_bit_cast(_Float16, (uint16_t)(rg >> 16));
                    const float sb = (float)__builtin_bit_cast(_Float16, (uint16_t)(S.b[slot] & 0xffffu));
                    const float alpha = 1.0f - expf(-sg * dt);
                    const float T = 1 - ws;
                    const float w = alpha * T;
                    ws += w;
                    t_c += delta1;
                    dep = fmaf(w, t_c, dep);
                    cr = fmaf(w, sr, cr); cg = fmaf(w, sgc, cg); cb = fmaf(w, sb, cb);
                    if (spec && (s0 + k + 1) % spec == 0) last_t = t_c;   // the next iteration's march_rays restarts its delta chain from rays_t
                    if ((double)T < 1e-4) break;             // :890: this sample does not count as a completed step
                }
                steps_done += k;
                if (k < want) running = false;               // early stop, or deltas[0] == 0 (march ran out of samples)
            } else if (do_march && cnt) {
                // keep the march's last_t chain consistent for a terminated ray that is still being dumped
                last_t = S.t[lane * kCh + cnt - 1] + S.dt[lane * kCh + cnt - 1];
            }
            if (ra.last_sigmas && active && !spec) {   // (a multi-iteration launch is never the reference's last iteration)
                for (uint32_t k = 0; k < want; k++) {
                    const uint32_t slot = lane * kCh + k;
                    if (k < cnt)
                        dump_row(ra, entry, ray, n_step, s0 + k, S.sig[slot], (float)__builtin_bit_cast(_Float16, (uint16_t)(S.rg[slot] & 0xffffu)),
                                 (float)__builtin_bit_cast(_Float16, (uint16_t)(S.rg[slot] >> 16)),
                                 (float)__builtin_bit_cast(_Float16, (uint16_t)(S.b[slot] & 0xffffu)));
                    else
                        dump_row(ra, entry, ray, n_step, s0 + k, ra.pad_sigma, ra.pad_r, ra.pad_g, ra.pad_b);
                }
            }
            NGP_STAMP(2)
            if (!ra.last_sigmas && !__any(running)) break;
        }
        // rows of sub-passes skipped after the whole wave stopped (dump mode never skips, so nothing to fill here)

        // ---- 4. write back state, chunk-local stable compaction of survivors
        const bool survive = active && running && steps_done == n_step;
        if (active) {
            if (survive) ra.rays_t[ray] = t_c;
            if (ra.sample_hash) {
                // diagnostics: FNV hash of the (dt, deltas[1]) bit patterns of the samples the reference marches for this ray in this
                // launch -- all n_step of every iteration it enters alive, composited or not (march_rays runs before composite_rays)
                const uint32_t entered = (spec && !survive) ? (steps_done / spec + 1) * spec : n_step;
                const uint32_t n_hash = emitted < entered ? emitted : entered;
                uint32_t hsh = ra.sample_hash[ray];
                float lm = t_start, gtc = t_c0;       // the march's last_t and the re-accumulated rays_t, as k_march_ahead carries them
                for (uint32_t i = 0; i < n_hash; i++) {
                    const float2 v = marched[(size_t)i * 64];
                    const float ta = v.x + v.y, d1 = ta - lm;
                    lm = ta;
                    hsh = (hsh ^ __float_as_uint(v.y)) * 16777619u;
                    hsh = (hsh ^ __float_as_uint(d1)) * 16777619u;
                    gtc += d1;
                    if (spec && (i + 1) % spec == 0) lm = gtc;
                }
                ra.sample_hash[ray] = hsh;
            }
            ra.weights_sum[ray] = ws; ra.depth[ray] = dep;
            ra.image[(size_t)ray * 3] = cr; ra.image[(size_t)ray * 3 + 1] = cg; ra.image[(size_t)ray * 3 + 2] = cb;
        }
        // Rays whose next march begins inside an empty 4x4x4 block are about to skip through empty space (tens of DDA
        // probes) while the others take one probe per sample.  Grouping them into their own chunks keeps the lanes of a
        // wave doing comparable work (measured lane utilisation of the march without this: 19 %).  The order of the alive
        // list does not enter any result (perturb == 0), so this is a pure scheduling decision.
        const bool slow = ra.sort_slow && survive && slow_next;      // (k_march_ahead looked the ray's next start position up)
        const unsigned long long ball_f = __ballot(survive && !slow), ball_s = __ballot(survive && slow);
        const unsigned long long lt_mask = (1ull << lane) - 1ull;
        if (survive && !slow) ra.staging[(size_t)first_entry + (uint32_t)__popcll(ball_f & lt_mask)] = ray;
        if (survive && slow) ra.staging[(size_t)first_entry + W - 1 - (uint32_t)__popcll(ball_s & lt_mask)] = ray;   // filled from the back
        if (lane == 0) ra.chunk_count[chunk] = (uint32_t)__popcll(ball_f) | ((uint32_t)__popcll(ball_s) << 16);
        if (spec) {
            // a ray that completed m samples died in the launch's m-th iteration: the n_alive sequence follows from these counts.
            const uint32_t ds = ((blockIdx.x * kWaves + wid) % kDeathShards) * kSpecK;
            for (uint32_t m = 0; m < n_step / spec; m++) {
                const uint32_t cdead = (uint32_t)__popcll(__ballot(active && !survive && steps_done / spec == m));
                if (lane == 0 && cdead) atomicAdd(&ra.death_shards[ds + m], cdead);
            }
        }
        if (ra.forecast) {
            // Saturation forecast, for the sizing of the NEXT launch only (k_render_compact, plan_launch): after how many further samples
            // does this survivor's T = 1 - ws fall below 1e-4 if the opacity of its last sample persists?  1 .. 8 are counted per wave
            // (ballots, as the deaths are) into the launch's forecast shards; anything later, and rays whose last sample was empty, are not.
            // (that sample's sigma and dt are still in the wave's slab: a survivor composited the last slot of the last sub-pass)
            uint32_t fb = 0;
            const uint32_t last_slot = lane * kCh + (n_step - 1u) % (uint32_t)kCh;
            const float alpha_last = survive ? 1.0f - expf(-S.sig[last_slot] * S.dt[last_slot]) : 0.0f;
            if (alpha_last > 0.0f) {
                const float x = ceilf(__logf(1e-4f / (1.0f - ws)) / __logf(1.0f - alpha_last));
                if (x <= (float)kForecastBuckets) fb = x < 1.0f ? 1u : (uint32_t)x;     // (NaN: not counted)
            }
            if (__any(fb != 0u)) {
                uint32_t* fc = ra.death_shards + kForecastAt + ((blockIdx.x * kWaves + wid) % kDeathShards) * kForecastBuckets;
                for (uint32_t s = 1; s <= kForecastBuckets; s++) {
                    const uint32_t n = (uint32_t)__popcll(__ballot(fb == s));
                    if (lane == 0 && n) atomicAdd(&fc[s - 1], n);
                }
            }
        }
        {
            // samples the reference marches for this ray: all of every iteration it enters alive (march_rays runs before
            // composite_rays); in a multi-iteration launch a ray that completed steps_done samples entered iterations 0 .. steps_done / spec
            const uint32_t entered = (spec && !survive) ? (steps_done / spec + 1) * spec : n_step;
            uint32_t rm = active ? (emitted < entered ? emitted : entered) : 0u;
#pragma unroll      // (wave_sum, written out since the refactor that compared ISA)
            for (int off = 32; off > 0; off >>= 1) rm += __shfl_xor(rm, off, 64);
            wave_samples = (uint32_t)__builtin_amdgcn_readfirstlane((int)rm);   // (wave-uniform after the reduction: the running total stays scalar)
        }
        wave_total += wave_samples;
        // padding rows of the reference's [M_padded] tensors (M += 128 - M % 128), written by the last chunk's wave
        if (ra.dump_iter && active) ra.dump_iter[ray] = ctl.iters;
        if (ra.last_sigmas && !ra.dump_rec && !spec && chunk == n_chunks - 1) {   // (never from a multi-iteration launch: its n_alive * n_step exceeds the tensors)
            for (uint32_t i = lane; i < 128; i += 64) {
                const size_t row = (size_t)n_alive * n_step + i;
                ra.last_sigmas[row] = ra.pad_sigma;
                ra.last_rgbs[row * 3] = ra.pad_r; ra.last_rgbs[row * 3 + 1] = ra.pad_g; ra.last_rgbs[row * 3 + 2] = ra.pad_b;
            }
        }
        NGP_STAMP(3)
    }
#undef NGP_STAMP
    if (lane == 0 && wave_total) atomicAdd(&ra.stat_shards[(blockIdx.x * kWaves + wid) % kStatShards], wave_total);
}

// stitch chunk survivor lists -> next alive list; its last thread advances the reference's schedule (renderer.py:347-373; finish_launch).
// One 256-thread block per 8 chunks (512 alive entries): wave w copies chunks 2w, 2w+1 of its block.  Survivors come in two
// classes per chunk (fast: stored from the front, slow: stored from the back, see k_render_iter); the next list is
// [all slow survivors in order | all fast survivors in order].  With no slow survivors this is the reference's stable
// compaction rays_alive[rays_alive >= 0].
// What the host needs while it enqueues iterations ahead -- how many rays are left and whether the loop has ended -- goes
// straight into its pinned, coherent status ring as ONE 64-bit word (pack_status), written
// with a relaxed system-scope store: no copy, no event, and no release fence (a fence writes the XCD's L2 back, ~10 us at the
// end of this short kernel).  Everything else the host reads from the device state after the loop.
// A state that ends the loop also leaves the counters the host reports (ngp_render_stats) in four more pinned words (pack_fin), each
// tagged with the render CALL: the run-ahead no-op launches of the previous call may still be writing their own, older tag when this
// call starts; the host takes the words once they carry this call's tag -- every launch of a call that publishes a finished state
// writes the same values, so there is nothing to tear -- the host then needs neither a stream synchronize nor a copy of the device
// state at the end of a frame, and the caller can enqueue the next frame's work at once.
__device__ __forceinline__ void publish_status(unsigned long long* host_slot, const Ctl& n, uint32_t seq, unsigned long long* fin = nullptr,
                                               uint32_t call_tag = 0) {
    if (!host_slot) return;
    if (n.done && fin) {
        unsigned long long w[4];
        pack_fin(n, call_tag, w);
        for (int i = 0; i < 4; i++) __hip_atomic_store(fin + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __hip_atomic_store(host_slot, pack_status(seq, n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// (Plain __restrict__ pointer arguments, not one struct by value: members of a struct cannot carry the qualifier, the uniform loads
//  of the launch's state and counts then become vector loads, and the kernel took 2.5 x as long -- DESIGN "One place for the schedule".)
__global__ void __launch_bounds__(256) k_render_compact(const Ctl* __restrict__ cur, Ctl* __restrict__ nxt, const int32_t* __restrict__ staging,
                                                         const uint32_t* __restrict__ chunk_count, int32_t* __restrict__ alive_out, uint32_t N,
                                                         uint32_t max_steps, unsigned long long* stat_shards, QueueHeads* __restrict__ nxt_heads,
                                                         unsigned long long* __restrict__ host_slot, uint32_t seq,
                                                         const uint32_t* __restrict__ death_shards, uint32_t flags, const int32_t* __restrict__ alive_in,
                                                         const float4* __restrict__ backup, float* __restrict__ rays_t, float* __restrict__ weights_sum,
                                                         float* __restrict__ depth, float* __restrict__ image, uint32_t* __restrict__ sample_hash,
                                                         uint32_t* __restrict__ death_next, uint32_t wave_slots,
                                                         unsigned long long* __restrict__ fin_host, uint32_t call_tag) {
    // The last thread of a launch hands the loop on: the next launch's counters start at zero, its state is stored and published.
    // (This launch's death counts are NOT cleared here: the other blocks of the kernel are still reading them for their verdict.
    // Launches alternate between two buffers; a buffer is cleared right before a multi-iteration launch uses it.)
    const auto hand_on = [&](const Ctl& n) {
        for (int i = 0; i < kStatShards; i++) stat_shards[i] = 0ull;       // per-launch sample counts: folded into n (or discarded)
        if (n.spec)   // the next launch counts deaths per iteration
            for (uint32_t i = 0; i < kForecastAt; i++) death_next[i] = 0;
        *nxt = n;
        for (int i = 0; i < 8; i++) nxt_heads->head[i][0] = 0;
        publish_status(host_slot, n, seq, fin_host, call_tag);
    };
    __shared__ uint32_t red[3][4];
    __shared__ uint32_t off_f[9], off_s[9];
    Ctl c = *cur;
    if (c.done) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            *nxt = c;
            publish_status(host_slot, c, seq, fin_host, call_tag);
        }
        return;
    }
    const uint32_t W = item_width(c.n_alive, wave_slots);
    const uint32_t n_chunks = (c.n_alive + W - 1) / W;      // k_render_iter's work items
    const uint32_t n_blocks = (n_chunks + 7) / 8;
    const uint32_t g = blockIdx.x;
    if (g >= n_blocks) return;
    const uint32_t first = g * 8;
    // ---- a launch that covered several reference iterations is verified first (every block reaches the same verdict) ----
    __shared__ uint32_t deaths[kSpecK], exhausted[kSpecK], forecast[kForecastBuckets];
    __shared__ uint32_t verdict_bad, verdict_keep;
    if (threadIdx.x < kSpecK) {
        uint32_t d = 0, x = 0;
        if (c.spec)
            for (int sh = 0; sh < kDeathShards; sh++) {
                d += death_shards[sh * kSpecK + threadIdx.x];
                x += death_shards[(size_t)kDeathShards * kSpecK + sh * kSpecK + threadIdx.x];
            }
        deaths[threadIdx.x] = d;
        exhausted[threadIdx.x] = x;
    } else if (threadIdx.x >= 64 && threadIdx.x < 128 && g == n_blocks - 1) {   // the forecast: read by the sizing code below, nothing else
        const uint32_t* f = death_shards + kForecastAt + (threadIdx.x - 64u) * kForecastBuckets;      // (wave 1, a shard per lane)
#pragma unroll
        for (uint32_t b = 0; b < kForecastBuckets; b++) {
            const uint32_t sum = wave_sum(f[b]);
            if (threadIdx.x == 64) forecast[b] = sum;
        }
    }
    __syncthreads();
    truncate_launch(c, exhausted, N);          // the launch k_render_iter actually ran (same counts, same cut)
    if (threadIdx.x == 0) {
        // K = c.n_step / q reference iterations of q = c.spec samples each, judged by launch_verdict (launch_plan.hpp)
        LaunchVerdict v = {0u, 0u};
        if (c.spec) v = launch_verdict(N, c.n_alive, c.spec, c.n_step / c.spec, deaths, (flags & kPlanOwnLast) != 0u);
        verdict_bad = v.bad;
        verdict_keep = v.keep;
    }
    __syncthreads();
    // the other parity's forecast shards start every launch at zero (its death counts: only a multi-iteration launch's, below)
    if (g == n_blocks - 1)
        for (uint32_t i = kForecastAt + threadIdx.x; i < kDeathWords; i += 256) death_next[i] = 0;
    if (verdict_bad) {
        // ROLLBACK: the launch was not equivalent to the reference's iterations.  Every ray it processed gets the state it
        // started from back, the alive list is handed on unchanged, and the iteration is run again on its own.
        for (uint32_t e = first * W + threadIdx.x; e < (first + 8) * W && e < c.n_alive; e += 256) {
            const int32_t ray = alive_in[e];
            const float4 a = backup[(size_t)ray * 2], b = backup[(size_t)ray * 2 + 1];
            rays_t[ray] = a.x; weights_sum[ray] = a.y; depth[ray] = a.z;
            if (sample_hash) sample_hash[ray] = __float_as_uint(a.w);
            image[(size_t)ray * 3] = b.x; image[(size_t)ray * 3 + 1] = b.y; image[(size_t)ray * 3 + 2] = b.z;
            alive_out[e] = ray;
        }
        if (g == n_blocks - 1 && threadIdx.x == 0) {
            unsigned long long lost = 0;                          // what the discarded launch cost
            for (int i = 0; i < kStatShards; i++) lost += stat_shards[i];
            hand_on(finish_launch(c, {1u, verdict_keep}, deaths, forecast, c.n_alive, lost, N, max_steps, flags, kSpecMidSamples, kSpecMaxSamples));
        }
        return;
    }
    uint32_t pf = 0, ps = 0, tf = 0;     // fast / slow survivors before this block, SLOW survivors in total
    for (uint32_t j = threadIdx.x; j < n_chunks; j += 256) {
        const uint32_t v = chunk_count[j];
        tf += v >> 16;
        if (j < first) { pf += v & 0xffffu; ps += v >> 16; }
    }
#pragma unroll      // (three wave_sum_lane0, interleaved, and a fourth below: written out since the refactor that compared ISA)
    for (int off = 32; off > 0; off >>= 1) {
        pf += __shfl_down(pf, off, 64);
        ps += __shfl_down(ps, off, 64);
        tf += __shfl_down(tf, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = pf; red[1][threadIdx.x >> 6] = ps; red[2][threadIdx.x >> 6] = tf; }
    if (threadIdx.x == 0) {
        uint32_t af = 0, as = 0;
        for (uint32_t i = 0; i < 8; i++) {
            const uint32_t v = (first + i < n_chunks) ? chunk_count[first + i] : 0;
            off_f[i] = af; off_s[i] = as;
            af += v & 0xffffu; as += v >> 16;
        }
        off_f[8] = af; off_s[8] = as;
    }
    __syncthreads();
    const uint32_t prefix_f = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const uint32_t prefix_s = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const uint32_t total_s = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        const uint32_t ci = w * 2 + h;
        const uint32_t nf = off_f[ci + 1] - off_f[ci], ns = off_s[ci + 1] - off_s[ci];
        // slow rays go FIRST: their chunks are the long jobs and must not form the tail of the work queue
        if (lane < ns) alive_out[prefix_s + off_s[ci] + lane] = staging[(size_t)(first + ci) * W + W - 1 - lane];
        if (lane < nf) alive_out[total_s + prefix_f + off_f[ci] + lane] = staging[(size_t)(first + ci) * W + lane];
    }
    unsigned long long marched = threadIdx.x < (uint32_t)kStatShards ? stat_shards[threadIdx.x] : 0ull;   // kStatShards == 64: wave 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) marched += __shfl_down(marched, off, 64);
    if (g == n_blocks - 1 && threadIdx.x == 0)
        hand_on(finish_launch(c, {0u, 0u}, deaths, forecast, total_s + prefix_f + off_f[8], marched, N, max_steps, flags, kSpecMidSamples, kSpecMaxSamples));
}

__global__ void __launch_bounds__(256) k_render_init(uint32_t N, const float* __restrict__ nears, float* __restrict__ rays_t,
                                                      int32_t* __restrict__ alive, float* __restrict__ weights_sum, float* __restrict__ depth,
                                                      float* __restrict__ image, Ctl* __restrict__ ctl, uint32_t max_steps,
                                                      uint32_t* __restrict__ sample_hash, unsigned long long* __restrict__ stat_shards,
                                                      QueueHeads* __restrict__ heads, uint32_t* __restrict__ death_shards, uint32_t flags,
                                                      uint32_t tile_w) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n < (uint32_t)kStatShards) stat_shards[n] = 0ull;
    if (n < 2u * kDeathWords) death_shards[n] = 0;   // both buffers (launches alternate between them)
    if (n < 16) heads[n >> 3].head[n & 7][0] = 0;
    if (n < N) {
        if (sample_hash) sample_hash[n] = 2166136261u;
        // the order of the alive list is free for perturb == 0 (see k_render_iter): with a known frame width the list starts in
        // 4x4-pixel tiles, so that the 16 samples of one MLP tile gather from neighbouring cells
        uint32_t first = n;
        if (tile_w) {
            const uint32_t t = n >> 4, in = n & 15u, per_row = tile_w >> 2;
            first = ((t / per_row) * 4u + (in >> 2)) * tile_w + (t % per_row) * 4u + (in & 3u);
        }
        alive[n] = (int32_t)first;
        rays_t[n] = nears[n];
        weights_sum[n] = 0; depth[n] = 0;
        image[(size_t)n * 3] = 0; image[(size_t)n * 3 + 1] = 0; image[(size_t)n * 3 + 2] = 0;
    }
    if (n == 0) {
        const Ctl c = loop_begin(N, max_steps, flags);
        ctl[0] = c;
        ctl[1] = c;
    }
}

// ---- restoring the reference's row order of the last iteration's tensors when the alive list was regrouped -------------
// The reference's alive list is always ascending in ray id (stable compaction of arange(N)), so row r of its last
// iteration belongs to the r-th smallest ray id that was alive then.  Three small launches after the loop: per-block counts
// of rays stamped with the last iteration, a one-block scan, and the scatter of the per-ray records.
__global__ void __launch_bounds__(256) k_dump_count(const uint32_t* __restrict__ dump_iter, uint32_t N, const Ctl* __restrict__ fin_state,
                                                     uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t ws[4];
    const uint32_t last_iter = fin_state->iters - 1;   // iters == 0 (nothing ran): the gather kernel returns at once
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    const bool f = n < N && dump_iter[n] == last_iter;
    const uint32_t c = (uint32_t)__popcll(__ballot(f));
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ void __launch_bounds__(1024) k_dump_scan(uint32_t* __restrict__ block_sums, uint32_t nblocks) {
    scan_in_place_1024(block_sums, nblocks);
}
__global__ void __launch_bounds__(256) k_dump_gather(const uint32_t* __restrict__ dump_iter, const float4* __restrict__ rec, uint32_t N,
                                                      const Ctl* __restrict__ fin_state, const uint32_t* __restrict__ block_off,
                                                      float* __restrict__ last_sigmas, float* __restrict__ last_rgbs, float ps, float pr, float pg,
                                                      float pb) {
    __shared__ uint32_t ws[4];
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (fin_state->iters == 0) return;   // no iteration ran: the caller takes nothing from the tensors
    const uint32_t last_iter = fin_state->iters - 1, n_alive = fin_state->last_n_alive, n_step = fin_state->last_n_step;
    const bool f = n < N && dump_iter[n] == last_iter;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) ws[wid] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t rank = block_off[blockIdx.x] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wid; w++) rank += ws[w];
    if (f) {
        for (uint32_t k = 0; k < n_step; k++) {
            const float4 v = rec[(size_t)n * 8 + k];
            const size_t row = (size_t)rank * n_step + k;
            last_sigmas[row] = v.x;
            last_rgbs[row * 3] = v.y; last_rgbs[row * 3 + 1] = v.z; last_rgbs[row * 3 + 2] = v.w;
        }
    }
    if (n < 128) {   // padding rows (M += 128 - M % 128)
        const size_t row = (size_t)n_alive * n_step + n;
        last_sigmas[row] = ps;
        last_rgbs[row * 3] = pr; last_rgbs[row * 3 + 1] = pg; last_rgbs[row * 3 + 2] = pb;
    }
}

}  // namespace ngp

using namespace ngp;

struct ngp_render_ctx {
    uint32_t max_rays = 0;
    uint32_t frame_width = 0;               // ngp_render_ctx_set_frame_width: rays are the pixels of row-major frames this wide (0: unknown)
    uint32_t sched_flags = 0;               // ngp_render_ctx_set_schedule_flags: NGP_SCHED_* switches of the launch sizing (diagnostics)
    const void* last_ctl = nullptr;         // the device state after the last launch of the most recent call, and its stream
    hipStream_t last_stream = nullptr;      // (ngp_render_ctx_schedule_stats)
    int32_t* alive[2] = {nullptr, nullptr};
    int32_t* staging = nullptr;
    uint32_t* chunk_count = nullptr;
    float* rays_t = nullptr;
    unsigned long long* coarse = nullptr;   // coarse occupancy bits (<= 8 KB)
    uint32_t* grid_lin = nullptr;           // x-fastest copy of the occupancy bitfield (k_build_linear), allocated on first use
    uint32_t* death_shards = nullptr;       // [kDeathShards][kSpecK] per-iteration death counts of a speculative launch
    float4* backup = nullptr;               // [max_rays][2] per-ray state a speculative launch starts from (for its rollback)
    float2* march_samples = nullptr;        // [(max_rays + 64) * 8] (t, dt) of the current launch's samples (k_march_ahead -> k_render_iter)
    uint8_t* march_counts = nullptr;        // [max_rays] samples marched per list entry + slow-ray flag
    float4* dump_rec = nullptr;             // lazily allocated: [max_rays][8]
    uint32_t* dump_iter = nullptr;          // [max_rays]
    Ctl* ctl = nullptr;          // device [2]
    unsigned long long* stat_shards = nullptr;
    QueueHeads* heads = nullptr;  // device [2]
    _Float16* packed = nullptr;  // device
    unsigned long long* status = nullptr;       // pinned, coherent [kRing] status words: written by k_render_compact, polled by the host
    unsigned long long* status_dev = nullptr;   // the same ring as the device addresses it
    unsigned long long* fin = nullptr;          // pinned, coherent [4]: the counters of a finished loop (publish_status)
    unsigned long long* fin_dev = nullptr;
    uint32_t calls = 0;                         // render calls made with this context (the tag of the words in `fin`)
    uint32_t seq_base = 0;       // sequence numbers already used by earlier render calls (slots are matched by number)
    hipEvent_t ev[kRing];
    int num_cu = 256;
    bool has_debug = false;      // ngp_render_ctx_set_debug: this context's own diagnostics state (else the process default)
    DebugState debug;
    void* owned[20] = {};        // every hipMalloc'ed buffer above (ctx_alloc), for ngp_render_ctx_destroy
    uint32_t n_owned = 0;
};

// hipMalloc into one of the context's pointers; the context owns the buffer from then on
template <typename T>
static bool ctx_alloc(ngp_render_ctx* c, T** p, size_t bytes) {
    if (c->n_owned == sizeof(c->owned) / sizeof(c->owned[0]) || hipMalloc(p, bytes) != hipSuccess) return false;
    c->owned[c->n_owned++] = *p;
    return true;
}

// this context's own diagnostics state (ngp_render_ctx_set_debug), else the process default
static DebugState debug_snapshot(const ngp_render_ctx* ctx) { return ctx->has_debug ? ctx->debug : ngp::debug_snapshot(); }

extern "C" {

int ngp_render_ctx_create(uint32_t max_rays, ngp_render_ctx** out) {
    NGP_REQUIRE(out, "render_ctx_create: null out pointer");
    NGP_REQUIRE(max_rays > 0, "render_ctx_create: max_rays must be positive");
    ngp_render_ctx* c = new ngp_render_ctx();
    c->max_rays = max_rays;
    const size_t chunks = div_up(max_rays, 64);
    bool ok = true;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    const size_t max_items = items_bound(max_rays, (uint32_t)c->num_cu * 16u) + 8;
    ok &= ctx_alloc(c, &c->alive[0], (size_t)max_rays * 4);
    ok &= ctx_alloc(c, &c->alive[1], (size_t)max_rays * 4);
    ok &= ctx_alloc(c, &c->staging, chunks * 64 * 4);
    ok &= ctx_alloc(c, &c->chunk_count, (max_items > (size_t)div_up(max_rays, 256) ? max_items : (size_t)div_up(max_rays, 256)) * 4);
    ok &= ctx_alloc(c, &c->rays_t, (size_t)max_rays * 4);
    ok &= ctx_alloc(c, &c->coarse, kCoarseMaxBytes);
    ok &= ctx_alloc(c, &c->ctl, 2 * sizeof(Ctl));
    ok &= ctx_alloc(c, &c->stat_shards, kStatShards * sizeof(unsigned long long));
    ok &= ctx_alloc(c, &c->death_shards, 2 * (size_t)kDeathWords * sizeof(uint32_t));   // two buffers, by launch parity
    ok &= ctx_alloc(c, &c->backup, (size_t)max_rays * 2 * sizeof(float4));
    // (n_alive * n_step <= 8 N in every regime of the schedule: n_step <= 8 while more than N / 5 rays live, <= 32 below that)
    ok &= ctx_alloc(c, &c->march_samples, ((size_t)max_rays + 512) * 8 * sizeof(float2));   // (n_alive / q + 64) * 8 q samples, q <= 4
    ok &= ctx_alloc(c, &c->march_counts, (size_t)max_rays);
    ok &= ctx_alloc(c, &c->heads, 2 * sizeof(QueueHeads));
    ok &= ctx_alloc(c, &c->packed, (size_t)(sig_halfs(2) + sig_halfs(3)) * 2);
    ok &= hipHostMalloc(&c->status, kRing * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (ok) {
        memset(c->status, 0, kRing * sizeof(unsigned long long));
        ok &= hipHostGetDevicePointer((void**)&c->status_dev, c->status, 0) == hipSuccess;
    }
    ok &= hipHostMalloc(&c->fin, 4 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (ok) {
        memset(c->fin, 0, 4 * sizeof(unsigned long long));
        ok &= hipHostGetDevicePointer((void**)&c->fin_dev, c->fin, 0) == hipSuccess;
    }
    for (int i = 0; i < kRing; i++) ok &= hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        set_error("render_ctx_create: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        ngp_render_ctx_destroy(c);
        return NGP_ENODEVICE;
    }
    *out = c;
    return NGP_OK;
}

int ngp_render_ctx_set_frame_width(ngp_render_ctx* ctx, uint32_t width) {
    NGP_REQUIRE(ctx, "render_ctx_set_frame_width: null context");
    ctx->frame_width = width;
    return NGP_OK;
}

int ngp_render_ctx_set_schedule_flags(ngp_render_ctx* ctx, uint32_t flags) {
    NGP_REQUIRE(ctx, "render_ctx_set_schedule_flags: null context");
    NGP_REQUIRE((flags & ~NGP_SCHED_NO_FORECAST) == 0, "render_ctx_set_schedule_flags: unknown bits 0x%x", flags);
    ctx->sched_flags = flags;
    return NGP_OK;
}

int ngp_render_ctx_schedule_stats(ngp_render_ctx* ctx, uint64_t* out) {
    NGP_REQUIRE(ctx && out, "render_ctx_schedule_stats: null pointer");
    Ctl fin = {};
    if (ctx->last_ctl &&
        (hipStreamSynchronize(ctx->last_stream) != hipSuccess || hipMemcpy(&fin, ctx->last_ctl, sizeof(Ctl), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("render_ctx_schedule_stats: %s", hipGetErrorString(hipGetLastError()));
        return NGP_ELAUNCH;
    }
    out[0] = fin.rollbacks; out[1] = fin.discarded; out[2] = 0; out[3] = fin.fc_sized;
    out[4] = fin.fc_pred; out[5] = fin.fc_actual; out[6] = fin.spec_launches; out[7] = 0;
    return NGP_OK;
}

int ngp_render_ctx_destroy(ngp_render_ctx* c) {
    if (!c) return NGP_OK;
    (void)hipDeviceSynchronize();      // a render call no longer ends with a synchronize: its run-ahead launches may still use the scratch
    for (uint32_t i = 0; i < c->n_owned; i++) (void)hipFree(c->owned[i]);
    if (c->status) (void)hipHostFree(c->status);
    if (c->fin) (void)hipHostFree(c->fin);
    for (int i = 0; i < kRing; i++) (void)hipEventDestroy(c->ev[i]);
    delete c;
    return NGP_OK;
}

// Render calls in progress in this process (a scheduling hint only: see the persistent workgroup count in enqueue_launch)
static std::atomic<int> g_active_renders{0};
struct ActiveRender {
    ActiveRender() { g_active_renders.fetch_add(1, std::memory_order_relaxed); }
    ~ActiveRender() { g_active_renders.fetch_sub(1, std::memory_order_relaxed); }
};

// The occupancy bits the march probes through: the linear copies (LIN kernels) when the grid has them and they fit this context's
// buffers, else the Morton-order coarse filter when the bitfield is 8-byte aligned and its 1:64 reduction fits the LDS budget, else the
// plain probes -- and then no regrouping of slow rays, which needs the coarse bits.  Returns whether the LIN kernels run.
static bool choose_occupancy(ngp_render_ctx* ctx, const ngp_model* model, const DebugState& dbg, hipStream_t s, RenderArgs& ra) {
    const uint32_t C = model->cascade, H = model->grid_size;
    const size_t cells = (size_t)C * H * H * H;
    // (NGP_DBG_NO_LIN turns the linear re-layout off; without the coarse filter there is none either)
    bool lin = !dbg.coarse_off() && !dbg.lin_off() && occupancy_lin_fits(C, H, model->density_bitfield, kLinMaxBytes, kCoarseMaxBytes);
    // (the Morton-order filter asks less of the grid: any H whose block bits fit)
    const bool use_coarse = !dbg.coarse_off() && cells % 4096 == 0 && cells / 64 / 8 <= kCoarseMaxBytes && ((uintptr_t)model->density_bitfield & 7) == 0;
    if (lin && !ctx->grid_lin && !ctx_alloc(ctx, &ctx->grid_lin, kLinMaxBytes)) lin = false;
    if (lin) {
        ra.occ = build_occupancy_lin(model->density_bitfield, C, H, ctx->grid_lin, ctx->coarse, s);
        ra.block_jump = dbg.jump_off() ? 0u : 1u;
    } else if (use_coarse) {
        const uint32_t n_words = (uint32_t)(cells / 64);
        k_build_coarse<<<div_up(n_words, 256), 256, 0, s>>>((const unsigned long long*)model->density_bitfield, n_words, ctx->coarse);
        ra.occ.coarse = (const uint32_t*)ctx->coarse;
        ra.occ.coarse_words = n_words / 32;
    } else {
        ra.sort_slow = 0;
    }
    return lin;
}

// What a call's launches share: the loop's scratch (context), the grid (model), the schedule (arguments) and the diagnostics state.
// The caller's own pointers (rays, outputs, padding) are filled in by ngp_render_rays.
static void fill_render_args(const ngp_render_ctx* ctx, const ngp_model* model, const DebugState& dbg, uint32_t N, float dt_gamma,
                             uint32_t max_steps, uint32_t perturb, RenderArgs& ra) {
    ra.rays_t = ctx->rays_t;
    ra.staging = ctx->staging; ra.chunk_count = ctx->chunk_count; ra.stat_shards = ctx->stat_shards;
    ra.wave_slots = dbg.narrow_items_off() ? 0u : (uint32_t)ctx->num_cu * 16u;
    ra.pre_verdict = dbg.pre_verdict_off() ? 0u : 1u;
    ra.cell_runs = dbg.cell_runs_off() ? 0u : 1u;
    ra.wave_march_max = (dbg.wave_march_off() || dt_gamma != 0.0f) ? 0u : (uint32_t)ctx->num_cu * 64u;
    ra.backup = ctx->backup;
    ra.march_samples = ctx->march_samples; ra.march_counts = ctx->march_counts;
    ra.bitfield = model->density_bitfield; ra.cascade = model->cascade; ra.grid_size = model->grid_size;
    ra.max_steps = max_steps; ra.perturb = perturb; ra.dt_gamma = dt_gamma;
    ra.n_rays = N;
    ra.rng.seed((uint64_t)perturb);  // raymarching.cu:819
    ra.stamps = dbg.stamps;
    ra.sort_slow = (perturb == 0 && !dbg.sort_off()) ? 1u : 0u;   // needs the coarse filter: choose_occupancy clears it without
    ra.sample_hash = dbg.sample_hash;
}

// the kernel instantiation of a call: (index recipe) x (corner rounding), and for the per-cell-record recipe x (out-of-range test
// compiled out when 2*bound is a power of two).  Only that recipe gets the third axis: it is the one the render loop is tuned for, and
// every instantiation costs this unit's compile time.
typedef void (*IterKernel)(NetArgs, GridLevels, RenderArgs);
static IterKernel choose_iter_kernel(const NetArgs& na, const GridLevels& lv) {
    static const IterKernel kIter[2][3] = {{k_render_iter<0, false>, k_render_iter<1, false>, k_render_iter<2, false>},
                                           {k_render_iter<0, true>, k_render_iter<1, true>, k_render_iter<2, true>}};
    static const IterKernel kIterClamped[2] = {k_render_iter<2, false, true>, k_render_iter<2, true, true>};
    const int mode = needs_generic(lv) ? 1 : (na.cells ? 2 : 0);
    if (mode == 2 && clamped_exact(na)) return kIterClamped[na.hacc() ? 1 : 0];
    return kIter[na.hacc() ? 1 : 0][mode];
}

// Enqueues launch number `launched` of a call: the march, the network over its samples, the compaction that publishes its status word.
// `ub`: the host's upper bound of the launch's n_alive.
static void enqueue_launch(ngp_render_ctx* ctx, const NetArgs& na, const GridLevels& lv, RenderArgs& ra, IterKernel iter_kernel, size_t lds,
                           bool lin, uint32_t ub, uint32_t launched, uint32_t plan_flags, uint32_t call_tag, hipStream_t s) {
    const uint32_t cur = launched & 1;
    const uint32_t chunks = items_bound(ub, ra.wave_slots);     // work items of the launch, at most
    // persistent: resident workgroups pull chunks from a queue.  k_render_iter at two workgroups per CU holds every vector register and
    // 144 KB of the LDS of the CUs it runs on, so nothing of another frame's launches runs beside it; at five eighths of that it
    // is 5 % slower on its own (its bound is the gather, not the waves in flight) and leaves room for another call's march and
    // compaction kernels: +2-3 % frames/s with three calls in flight.  Taken when another render call of this process is in progress
    // (results do not depend on the workgroup count).
    const uint32_t blocks_per_cu = lds <= 80 * 1024 ? 2 : 1;
    const uint32_t blocks_pct = g_active_renders.load(std::memory_order_relaxed) > 1 ? 62u : 100u;
    const uint32_t max_blocks = (uint32_t)ctx->num_cu * blocks_per_cu * blocks_pct / 100u;
    const uint32_t want_blocks = div_up(chunks, kWaves);
    const uint32_t blocks = want_blocks < max_blocks ? want_blocks : max_blocks;
    ra.alive_in = ctx->alive[cur];
    ra.ctl = ctx->ctl + cur;
    ra.heads = ctx->heads + cur;
    ra.death_shards = ctx->death_shards + (size_t)cur * kDeathWords;
    {
        ProfScope pm("k_march_ahead", s, 0);  // per-launch events only when ngp_prof_enable(1)
        // (one wave per ray when the launch turns out to have at most wave_march_max rays: four rays per block)
        const uint32_t by_wave = div_up(ub < ra.wave_march_max ? ub : ra.wave_march_max, 4);
        const uint32_t by_lane = div_up(ub ? ub : 1, 256);
        if (lin) k_march_ahead<true><<<by_lane > by_wave ? by_lane : by_wave, 256, 0, s>>>(ra, na.bound);
        else k_march_ahead<false><<<div_up(ub ? ub : 1, 256), 256, 0, s>>>(ra, na.bound);
    }
    {
        ProfScope pk("k_render_iter", s, 0);
        iter_kernel<<<blocks, kThreads, lds, s>>>(na, lv, ra);
    }
    k_render_compact<<<div_up(chunks, 8), 256, 0, s>>>(ra.ctl, ctx->ctl + (cur ^ 1), ra.staging, ra.chunk_count, ctx->alive[cur ^ 1], ra.n_rays,
                                                       ra.max_steps, ra.stat_shards, ctx->heads + (cur ^ 1), ctx->status_dev + launched % kRing,
                                                       ctx->seq_base + launched + 1, ra.death_shards, plan_flags, ra.alive_in, ra.backup, ra.rays_t,
                                                       ra.weights_sum, ra.depth, ra.image, ra.sample_hash,
                                                       ctx->death_shards + (size_t)(cur ^ 1) * kDeathWords, ra.wave_slots, ctx->fin_dev, call_tag);
}

// NGP_TRACE_SCHEDULE: one line per multi-iteration launch -- its plan (K iterations of q samples, what the death rate alone would have
// taken, the headroom, the per-iteration guess, the forecast deaths before the last verified iteration), what happened (deaths and
// march-exhausted rays per iteration) and whether it was rolled back.  Waits for the launch: the trace serialises host
// and device, the schedule itself is the device's and does not change.
static void trace_launch(const ngp_render_ctx* ctx, hipStream_t s, uint32_t launch, uint32_t call_tag) {
    const uint32_t cur = launch & 1;
    Ctl in = {}, out = {};
    uint32_t words[kDeathWords];
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(&in, ctx->ctl + cur, sizeof(Ctl), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&out, ctx->ctl + (cur ^ 1), sizeof(Ctl), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(words, ctx->death_shards + (size_t)cur * kDeathWords, sizeof(words), hipMemcpyDeviceToHost) != hipSuccess)
        return;
    if (in.done || !in.spec) return;
    const uint32_t q = in.spec, K = in.n_step / q;
    char deaths[128] = "", gone[128] = "";
    size_t nd = 0, ng = 0;
    for (uint32_t j = 0; j < K && j < kSpecK; j++) {
        uint32_t d = 0, x = 0;
        for (int sh = 0; sh < kDeathShards; sh++) { d += words[sh * kSpecK + j]; x += words[kDeathShards * kSpecK + sh * kSpecK + j]; }
        nd += (size_t)snprintf(deaths + nd, sizeof(deaths) - nd, "%s%u", j ? "," : "", d);
        ng += (size_t)snprintf(gone + ng, sizeof(gone) - ng, "%s%u", j ? "," : "", x);
    }
    fprintf(stderr, "[ngp] plan {\"call\": %u, \"launch\": %u, \"n_alive\": %u, \"q\": %u, \"K\": %u, \"K_rate\": %u, \"headroom\": %u, \"rate\": %u, "
            "\"forecast\": %u, \"deaths\": [%s], \"exhausted\": [%s], \"cut_short\": %u, \"rolled_back\": %u, \"n_alive_after\": %u}\n",
            call_tag, launch + 1, in.n_alive, q, K, in.plan_k_rate, in.plan_headroom, in.plan_rate, in.plan_pred, deaths, gone, out.rsv - in.rsv,
            out.rollbacks - in.rollbacks, out.n_alive);
}

// Consumes every status word that has already landed (known -> launched); blocks only when the host is kLookahead launches ahead.
// Each word gives the next launch's bound `ub`, the last one sets `done`.
static int consume_status(const ngp_render_ctx* ctx, hipStream_t s, uint32_t launched, uint32_t call_tag, bool trace, uint32_t& known,
                          uint32_t& ub, bool& done) {
    while (known < launched) {
        const bool must_wait = launched - known >= (uint32_t)kLookahead;
        volatile unsigned long long* slot = ctx->status + known % kRing;
        const uint32_t want_seq = ctx->seq_base + known + 1;
        unsigned long long w = *slot;
        if (unpack_status(w).seq != want_seq) {
            if (!must_wait) break;
            uint32_t spins = 0;
            while (unpack_status(w = *slot).seq != want_seq) {
                // every 2^20 polls (tens of milliseconds: far longer than any launch) make sure the stream is still alive.  Rarely,
                // because the query is not free on the device side: the runtime answers it with a marker packet in the queue, and the
                // kernels behind it start ~6 us late -- at every 4096 polls that was one gap per launch (kernel timeline, round 3)
                if ((++spins & 0xFFFFFu) == 0) {
                    const hipError_t q = hipStreamQuery(s);
                    if (q != hipSuccess && q != hipErrorNotReady) {
                        set_error("render_rays: %s", hipGetErrorString(q));
                        return NGP_ELAUNCH;
                    }
                    if (q == hipSuccess && unpack_status(*slot).seq != want_seq) {   // everything ran, nothing was published: cannot happen
                        set_error("render_rays: the device finished without publishing iteration %u", known);
                        return NGP_ELAUNCH;
                    }
                }
                __builtin_ia32_pause();
            }
        }
        known++;
        const LoopStatus st = unpack_status(w);
        ub = st.n_alive;
        if (trace) fprintf(stderr, "[ngp] call %u launch %u: n_alive %u%s\n", call_tag, known, ub, st.done ? " done" : "");
        if (st.done) { done = true; break; }
    }
    return NGP_OK;
}

// The finished loop's counters -> *stats_host (and, with `sync`, the wait for the stream).  `last`: the Ctl after the last launch.
static int read_counters(const ngp_render_ctx* ctx, hipStream_t s, const Ctl* last, uint32_t call_tag, uint32_t N, uint32_t launches, int sync,
                         ngp_render_stats* stats_host) {
    bool have_fin = false;
    Ctl fin = {};   // state after the last enqueued iteration (done is sticky)
    if (stats_host && !sync) {
        // the finished loop's counters arrive in pinned memory next to the status word the loop has already seen: a short,
        // bounded wait for the four tags (they are stored just before that word), then no synchronize and no copy
        volatile unsigned long long* f = ctx->fin;
        unsigned long long w[4] = {0, 0, 0, 0};
        for (uint32_t spin = 0; spin < 200000u && !have_fin; spin++) {
            for (int i = 0; i < 4; i++) w[i] = f[i];
            have_fin = unpack_fin(w, call_tag, fin);
            if (!have_fin) __builtin_ia32_pause();
        }
    }
    if ((stats_host && !have_fin) || sync) {
        if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(&fin, last, sizeof(Ctl), hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("render_rays: %s", hipGetErrorString(hipGetLastError()));
            return NGP_ELAUNCH;
        }
        have_fin = true;
    }
    if (have_fin && stats_host) {
        stats_host->samples_marched = fin.samples_marched;
        stats_host->samples_slots = fin.samples_slots;
        stats_host->iterations = fin.iters;
        stats_host->rays = N;
        stats_host->last_n_alive = fin.last_n_alive;
        stats_host->last_n_step = fin.last_n_step;
        stats_host->launches = launches;
        stats_host->replayed = fin.rollbacks;
        prof_add_units("k_render_iter", (double)fin.samples_marched);
    }
    return NGP_OK;
}

int ngp_render_rays(ngp_render_ctx* ctx, const ngp_model* model, const float* rays_o, const float* rays_d, const float* nears,
                    const float* fars, uint32_t N, float dt_gamma, uint32_t max_steps, uint32_t perturb, float* weights_sum, float* depth,
                    float* image, float* last_sigmas, float* last_rgbs, const float* pad_value_host, ngp_render_stats* stats_host, int sync,
                    ngp_stream_t stream) {
    NGP_REQUIRE(ctx, "render_rays: null context");
    NGP_REQUIRE(N <= ctx->max_rays, "render_rays: %u rays exceed the context capacity %u", N, ctx->max_rays);
    NGP_REQUIRE((last_sigmas == nullptr) == (last_rgbs == nullptr), "render_rays: last_sigmas and last_rgbs must both be given or both NULL");
    if (stats_host) *stats_host = ngp_render_stats{};
    if (N == 0) return NGP_OK;
    const ActiveRender active_render;
    NGP_REQUIRE(rays_o && rays_d && nears && fars && weights_sum && depth && image, "render_rays: null pointer");
    NGP_REQUIRE(model && model->density_bitfield, "render_rays: model has no density bitfield");
    NGP_REQUIRE(model->cascade >= 1 && model->cascade <= 8 && grid_size_ok(model->grid_size),
                "render_rays: unsupported cascade/grid size C=%u H=%u (C in [1, 8]; " NGP_GRID_SIZE_RULE ")", model->cascade, model->grid_size);
    hipStream_t s = (hipStream_t)stream;
    const DebugState dbg = debug_snapshot(ctx);   // ONE snapshot per call (see DebugState)
    NetArgs na;
    GridLevels lv;
    // fragment-major weights: the model's own (ngp_pack_weights, packed once per parameter version) or, without them, packed into
    // this context's buffer now
    const _Float16* packed = model && model->packed_weights ? (const _Float16*)model->packed_weights : ctx->packed;
    int rc = fill_net(model, packed, na, lv);
    if (rc) return rc;
    NGP_REQUIRE(!na.f32(), "render_rays: the occupancy-grid loop is built for the fp16 network (ngp_model::precision == NGP_PREC_F16)");
    if (!model->packed_weights) {
        const uint32_t n_packed = sig_halfs(na.sig_mm) + sig_halfs(na.col_mm);
        k_pack_weights<<<div_up(n_packed, 256), 256, 0, s>>>((const _Float16*)model->sigma_weights, na.sig_mm,
                                                             (const _Float16*)model->color_weights, na.col_mm, ctx->packed);
    }
    // several reference iterations per launch (launch_plan.hpp), not with jitter
    const uint32_t plan_flags = (!dbg.spec_off() && perturb == 0)
                                    ? (kPlanMulti | (last_sigmas ? kPlanOwnLast : 0u) | (dbg.prefix_replay_off() ? kPlanReplayOne : 0u) |
                                       ((ctx->sched_flags & NGP_SCHED_NO_FORECAST) ? kPlanNoForecast : 0u)) : 0u;
    // scheduling hint (ngp_render_ctx_set_frame_width): whole rows of 4x4-pixel tiles only; not with jitter (seeded with the list index)
    const uint32_t fw = ctx->frame_width;
    const uint32_t tile_w = (perturb == 0 && !dbg.tile_off() && fw >= 4 && fw % 4 == 0 && N % (4 * fw) == 0) ? fw : 0u;
    // (the grid also has to cover the loop's own counters -- both death-count buffers -- however few rays there are)
    const uint32_t init_threads = N > 2u * kDeathWords ? N : 2u * kDeathWords;
    k_render_init<<<div_up(init_threads, 256), 256, 0, s>>>(N, nears, ctx->rays_t, ctx->alive[0], weights_sum, depth, image, ctx->ctl, max_steps,
                                                 dbg.sample_hash, ctx->stat_shards, ctx->heads, ctx->death_shards, plan_flags, tile_w);

    RenderArgs ra = {};
    ra.rays_o = rays_o; ra.rays_d = rays_d; ra.fars = fars;
    ra.weights_sum = weights_sum; ra.depth = depth; ra.image = image;
    ra.last_sigmas = last_sigmas; ra.last_rgbs = last_rgbs;
    if (pad_value_host) { ra.pad_sigma = pad_value_host[0]; ra.pad_r = pad_value_host[1]; ra.pad_g = pad_value_host[2]; ra.pad_b = pad_value_host[3]; }
    fill_render_args(ctx, model, dbg, N, dt_gamma, max_steps, perturb, ra);
    ra.forecast = ((plan_flags & kPlanMulti) && !(plan_flags & kPlanNoForecast)) ? 1u : 0u;         // (ngp_render_ctx_set_schedule_flags)
    const bool lin = choose_occupancy(ctx, model, dbg, s, ra);
    if ((ra.sort_slow || tile_w) && last_sigmas) {
        // regrouped alive list + last-iteration tensors requested: collect per-ray records, restore the row order afterwards
        if (!ctx->dump_rec) {
            if (!ctx_alloc(ctx, &ctx->dump_rec, (size_t)ctx->max_rays * 8 * sizeof(float4)) ||
                !ctx_alloc(ctx, &ctx->dump_iter, (size_t)ctx->max_rays * 4)) {
                set_error("render_rays: cannot allocate the per-ray record buffer");
                return NGP_ENODEVICE;
            }
        }
        (void)hipMemsetAsync(ctx->dump_iter, 0xff, (size_t)N * 4, s);
        ra.dump_rec = ctx->dump_rec;
        ra.dump_iter = ctx->dump_iter;
    }
    const size_t lds = weights_bytes(na) + sizeof(LevelTab) + (size_t)kWaves * sizeof(WaveSlab);
    const IterKernel iter_kernel = choose_iter_kernel(na, lv);
    ensure_dynamic_lds(reinterpret_cast<const void*>(iter_kernel), 160 * 1024);
    NGP_REQUIRE(lds <= 160 * 1024, "render_rays: LDS budget exceeded (%zu bytes)", lds);

    const bool trace = env_set("NGP_TRACE_SCHEDULE");   // diagnostics: prints the alive count after every launch
    const uint32_t call_tag = ++ctx->calls & 0x7FFFu;
    uint32_t ub = N;          // host-side upper bound of n_alive
    uint32_t launched = 0;    // iterations enqueued
    uint32_t known = 0;       // iterations whose resulting status the host has read
    bool done = false;
    while (!done) {
        enqueue_launch(ctx, na, lv, ra, iter_kernel, lds, lin, ub, launched, plan_flags, call_tag, s);
        launched++;
        if (trace) trace_launch(ctx, s, launched - 1, call_tag);
        rc = consume_status(ctx, s, launched, call_tag, trace, known, ub, done);
        if (rc) return rc;
        if (launched > 2u * max_steps + 16u) {  // cannot happen: every launch advances step by >= 1 or is the rollback of one that did
            set_error("render_rays: iteration bound exceeded");
            return NGP_ELAUNCH;
        }
    }
    ctx->seq_base += launched;
    const Ctl* last = ctx->ctl + (launched & 1);   // the state after the last launch (done is sticky)
    ctx->last_ctl = last;
    ctx->last_stream = s;
    if (ra.dump_rec) {
        const uint32_t nb = div_up(N, 256);
        k_dump_count<<<nb, 256, 0, s>>>(ctx->dump_iter, N, last, ctx->chunk_count);
        k_dump_scan<<<1, 1024, 0, s>>>(ctx->chunk_count, nb);
        k_dump_gather<<<nb, 256, 0, s>>>(ctx->dump_iter, ctx->dump_rec, N, last, ctx->chunk_count,
                                         last_sigmas, last_rgbs, ra.pad_sigma, ra.pad_r, ra.pad_g, ra.pad_b);
    }
    rc = check_launch("render_rays");
    if (rc) return rc;
    return read_counters(ctx, s, last, call_tag, N, 2 + 3 * launched, sync, stats_host);
}

int ngp_render_ctx_set_debug(ngp_render_ctx* ctx, int enable, int flags, unsigned long long* stamps, uint32_t* sample_hash) {
    NGP_REQUIRE(ctx, "render_ctx_set_debug: null context");
    if (!debug_flags_valid(flags, "render_ctx_set_debug")) return NGP_EINVAL;
    ctx->has_debug = enable != 0;
    ctx->debug.flags = flags; ctx->debug.stamps = stamps; ctx->debug.sample_hash = sample_hash;
    return NGP_OK;
}

}  // extern "C"
