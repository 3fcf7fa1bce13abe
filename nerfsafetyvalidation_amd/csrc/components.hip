// components.hip -- connected-component labelling of a 3-D occupancy lattice (nerfsafetyvalidation_amd/collision.py,
// label_components / component_table): the primitive behind remove_floaters, floater_report and mesh.drop_small_components.
//
// The rule (collision.py's docstring has it in full): occupied uint8 [X,Y,Z] in C order, non-zero = occupied; two occupied cells are
// neighbours when their offset is one of the `connectivity` offsets (6 / 18 / 26: at most 1 / 2 / 3 non-zero entries of {-1,0,1}^3;
// 14: +- the seven Kuhn edges {0,1}^3 \ 0).  labels int32 [X,Y,Z] = 0 on empty cells, 1 + rank on the others, components ranked by
// the smallest C-order index of their cells; n = the number of components.  A function of the input alone.
//
// Every offset set is symmetric, so only its 13 "forward" members (the ones that raise the linear index) are ever walked: kFwd, with
// one bit per member and connectivity in the `fwd` mask.  The representative of a component is its cell of smallest linear index:
// every link of the union-find points from a cell to a cell of SMALLER index (or itself), which is what makes it a forest whatever
// the order of the atomics, and makes every chain strictly decreasing.
//
//   k_cc_tile     one workgroup per tile of kTX x kTY x kTZ = 4 x 4 x 16 cells, one lane per cell.  Union-find over the tile's cells in
//                 LDS (atomicMin on LDS words), then parent[cell] = the linear index of the cell's tile-local root (-1 on an empty
//                 cell).  A box's local C order agrees with the global one, so the local root is the tile's smallest cell.
//   k_cc_seams    one lane per cell: for every forward neighbour in ANOTHER tile, union the two cells on `parent` in global memory.
//                 Find follows parent[] to a fixed point, union hooks the larger root under the smaller with atomicMin and carries
//                 on from the value it displaced when it lost a race.
//   k_cc_flatten  labels[cell] = find(cell) (-1 on empty cells), shortening parent[cell] on the way; counts the roots (find == cell)
//                 of each block of kScanCells cells into sums[block].
//   k_cc_scan     ONE workgroup: sums[] -> its exclusive prefix sum in place; the total is n -> *n_components.
//   k_cc_rank     roots only: parent[root] = 1 + sums[block] + the roots before it in its block (ballot + popcount, C order).
//   k_cc_relabel  labels[cell] = parent[labels[cell]] (0 on empty cells).
//
// Memory visibility.  No workgroup ever waits for another: there is no flag, ticket or spin anywhere.  Within one launch only
// `parent` is both written and read by different workgroups (k_cc_seams, k_cc_flatten): every read of it there is
// __hip_atomic_load(.., relaxed, agent scope) and every write an agent-scope atomicMin, so a reader never sees a stale line of
// another XCD's writer, and whatever value it sees is one that was stored -- an ancestor of the cell, which is all find needs.
// Everything else crosses a launch boundary on the one stream: `occupied` (read-only input), `labels` (each launch touches only a
// lane's own cell, except k_cc_relabel's read of `parent`, written by the launch before), `sums` (k_cc_flatten writes, k_cc_scan
// rewrites, k_cc_rank reads), the error word (atomicMax from any lane; read by k_cc_scan, a later launch).  k_cc_tile's LDS words
// are shared within the workgroup only: workgroup-scope atomics between __syncthreads().
//
// Loop bounds.  A chain visits strictly decreasing indices, so a find from cell c ends within c + 1 <= N steps (tile: kTileCells);
// a union's retry moves to the value it displaced, strictly below the root it tried to hook, so it ends within 2 N rounds (the
// larger of the two ends falls every round).  The loops carry exactly these bounds, N + 1 and 2 N + 2 -- they cannot trip on a sound
// `parent`, whatever the map (the one-cell-wide snake included: its chains are the longest there are, and shorter than N).  A lane
// that does reach one (a corrupted workspace) records its stage in the error word and leaves; k_cc_scan then reports -stage in
// *n_components in place of n, and ngp_component_stats refuses such an n with the stage's name.
//
// ngp_component_stats: one lane per cell, a wave per 16 consecutive chunks of 64 cells.  The lanes of a chunk that hold the same label
// are reduced in the wave first (ballot + shuffles: cells, overlap, the six box bounds); the wave keeps the result while the next
// group is of the same label and lets one lane issue the integer atomics (add on int64, min / max on int32) when the label changes
// -- a map that is one giant component sends one lane per 1024 cells to its row (with one lane per 64 cells the row's atomics
// serialised: 8.9 ms at 256^3, now 0.6 ms).  Integer atomics only: the result does not depend on their order.
#include <limits.h>

#include "ngp_common.hpp"
#include "wave_ops.hpp"

namespace ngp {

constexpr uint32_t kTX = NGP_COMPONENTS_TILE_X, kTY = NGP_COMPONENTS_TILE_Y, kTZ = NGP_COMPONENTS_TILE_Z;
constexpr uint32_t kTileCells = kTX * kTY * kTZ;      // = the workgroup size of k_cc_tile
constexpr uint32_t kCcBlock = 256;
constexpr uint32_t kScanPerThread = 4;
constexpr uint32_t kScanCells = kCcBlock * kScanPerThread;      // cells per block of k_cc_flatten / k_cc_rank: chunk j of a block is
                                                                // cells block * kScanCells + j * kCcBlock + thread
constexpr uint32_t kScanBlock = 1024;
constexpr uint32_t kStatsChunks = 16;          // chunks of 64 cells a wave of k_cc_stats walks
static_assert(kTileCells == kCcBlock, "k_cc_tile: one lane per tile cell");

enum CcStage { kStageTile = 1, kStageSeams = 2, kStageFlatten = 3 };
static const char* const kStageName[] = {"", "tile", "seams", "flatten"};

// the 13 forward offsets: (dx, dy, dz) lexicographically above (0, 0, 0)
constexpr int kNumFwd = 13;
__constant__ int8_t kFwd[kNumFwd][3] = {{0, 0, 1},  {0, 1, -1}, {0, 1, 0}, {0, 1, 1},  {1, -1, -1}, {1, -1, 0}, {1, -1, 1},
                                                         {1, 0, -1}, {1, 0, 0},  {1, 0, 1}, {1, 1, -1}, {1, 1, 0},   {1, 1, 1}};
static const int8_t kFwdHost[kNumFwd][3] = {{0, 0, 1},  {0, 1, -1}, {0, 1, 0}, {0, 1, 1},  {1, -1, -1}, {1, -1, 0}, {1, -1, 1},
                                            {1, 0, -1}, {1, 0, 0},  {1, 0, 1}, {1, 1, -1}, {1, 1, 0},   {1, 1, 1}};

// connectivity -> the mask of forward offsets it holds; 0 for anything but 6, 14, 18, 26
static uint32_t forward_mask(uint32_t connectivity) {
    uint32_t mask = 0;
    for (int k = 0; k < kNumFwd; k++) {
        const int8_t* o = kFwdHost[k];
        const int nnz = (o[0] != 0) + (o[1] != 0) + (o[2] != 0);
        bool in = false;
        switch (connectivity) {
            case 6: in = nnz == 1; break;
            case 18: in = nnz <= 2; break;
            case 26: in = true; break;
            case 14: in = o[0] >= 0 && o[1] >= 0 && o[2] >= 0; break;      // (the backward half holds the all-negative ones)
            default: break;
        }
        if (in) mask |= 1u << k;
    }
    return mask;
}

__device__ __forceinline__ void cc_fail(int32_t* err, int stage) { atomicMax(err, stage); }

// ---- union-find on LDS words (one workgroup) ----------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(const int* s, int c, bool& ok) {
    for (uint32_t step = 0; step <= kTileCells; step++) {
        const int p = lds_load(&s[c]);
        if (p == c) return c;
        c = p;
    }
    ok = false;
    return c;
}

__device__ __forceinline__ void lds_union(int* s, int a, int b, bool& ok) {
    for (uint32_t round = 0; round < 2 * kTileCells + 2; round++) {
        a = lds_find(s, a, ok);
        b = lds_find(s, b, ok);
        if (a == b || !ok) return;
        if (a < b) { const int t = a; a = b; b = t; }          // hook the larger root a under b
        const int old = atomicMin(&s[a], b);
        if (old == a) return;
        a = old;                                                   // a had been hooked meanwhile: carry on from where it points
    }
    ok = false;
}

// ---- union-find on `parent` in global memory (any workgroup): agent-scope atomics only ----------------------------------------------
__device__ __forceinline__ int32_t g_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t g_find(const int32_t* parent, int32_t c, uint32_t bound, bool& ok) {
    for (uint32_t step = 0; step < bound; step++) {
        const int32_t p = g_load(&parent[c]);
        if (p == c) return c;
        if (p < 0) break;          // (an empty cell's mark: never on an occupied cell's chain)
        c = p;
    }
    ok = false;
    return c;
}

__device__ __forceinline__ void g_union(int32_t* parent, int32_t a, int32_t b, uint32_t n, bool& ok) {
    const int32_t a0 = a, b0 = b;
    const uint32_t rounds = n < 0x7fffffffu ? 2 * n + 2 : 0xffffffffu;
    for (uint32_t round = 0; round < rounds; round++) {
        a = g_find(parent, a, n + 1, ok);
        b = g_find(parent, b, n + 1, ok);
        if (!ok) return;
        if (a == b) break;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(&parent[a], b);
        if (old == a) { a = b; break; }
        a = old;
        if (round + 1 == rounds) { ok = false; return; }
    }
    // shorten the two chains this lane walked: the root found is an ancestor of both, and atomicMin keeps the smaller ancestor
    atomicMin(&parent[a0], a);
    atomicMin(&parent[b0], a);
}

// ---- stage 1: a tile in LDS ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTileCells) k_cc_tile(const uint8_t* __restrict__ occ, uint32_t X, uint32_t Y, uint32_t Z, uint32_t tiles_y,
                                                        uint32_t tiles_z, uint32_t fwd, int32_t* __restrict__ parent, int32_t* err) {
    __shared__ int s_lab[kTileCells];
    __shared__ uint8_t s_occ[kTileCells];
    const uint32_t t = threadIdx.x;
    const uint32_t lz = t % kTZ, ly = (t / kTZ) % kTY, lx = t / (kTZ * kTY);
    const uint32_t tz = blockIdx.x % tiles_z, ty = (blockIdx.x / tiles_z) % tiles_y, tx = blockIdx.x / (tiles_z * tiles_y);
    const uint32_t x = tx * kTX + lx, y = ty * kTY + ly, z = tz * kTZ + lz;
    const bool in_map = x < X && y < Y && z < Z;
    const size_t cell = ((size_t)x * Y + y) * Z + z;
    const bool mine = in_map && occ[cell] != 0;
    s_occ[t] = mine;
    s_lab[t] = (int)t;
    __syncthreads();
    bool ok = true;
    if (mine) {
#pragma unroll
        for (int k = 0; k < kNumFwd; k++) {
            if (!((fwd >> k) & 1)) continue;
            const uint32_t nx = lx + kFwd[k][0], ny = ly + kFwd[k][1], nz = lz + kFwd[k][2];      // (a -1 wraps above the tile size)
            if (nx >= kTX || ny >= kTY || nz >= kTZ) continue;
            const uint32_t u = (nx * kTY + ny) * kTZ + nz;
            if (s_occ[u]) lds_union(s_lab, (int)t, (int)u, ok);
        }
    }
    __syncthreads();
    if (in_map) {
        int32_t p = -1;
        if (mine) {
            const uint32_t r = (uint32_t)lds_find(s_lab, (int)t, ok);
            const uint32_t rz = r % kTZ, ry = (r / kTZ) % kTY, rx = r / (kTZ * kTY);
            p = (int32_t)(((size_t)(tx * kTX + rx) * Y + (ty * kTY + ry)) * Z + (tz * kTZ + rz));
        }
        parent[cell] = p;
    }
    if (!ok) cc_fail(err, kStageTile);
}

// ---- stage 2: unions across tile faces ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcBlock) k_cc_seams(const uint8_t* __restrict__ occ, uint32_t X, uint32_t Y, uint32_t Z, uint32_t n, uint32_t fwd,
                                                       int32_t* parent, int32_t* err) {
    const uint32_t cell = blockIdx.x * kCcBlock + threadIdx.x;
    if (cell >= n || occ[cell] == 0) return;
    const uint32_t z = cell % Z, y = (cell / Z) % Y, x = cell / (Z * Y);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kNumFwd; k++) {
        if (!((fwd >> k) & 1)) continue;
        const uint32_t nx = x + kFwd[k][0], ny = y + kFwd[k][1], nz = z + kFwd[k][2];      // (a -1 at 0 wraps above every size)
        if (nx >= X || ny >= Y || nz >= Z) continue;
        if (nx / kTX == x / kTX && ny / kTY == y / kTY && nz / kTZ == z / kTZ) continue;      // k_cc_tile joined these
        const uint32_t other = (nx * Y + ny) * Z + nz;
        if (occ[other] != 0) g_union(parent, (int32_t)cell, (int32_t)other, n, ok);
    }
    if (!ok) cc_fail(err, kStageSeams);
}

// the number of set flags among the lanes below this one, and in the wave
__device__ __forceinline__ uint32_t flags_below(bool flag, uint32_t lane, uint32_t& in_wave) {
    const uint64_t m = __ballot(flag);
    in_wave = (uint32_t)__popcll(m);
    return (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// ---- stage 3: every cell to its root, and the roots of each block counted ------------------------------------------------------------
__global__ void __launch_bounds__(kCcBlock) k_cc_flatten(uint32_t n, int32_t* parent, int32_t* __restrict__ labels, uint32_t* __restrict__ sums,
                                                         int32_t* err) {
    __shared__ uint32_t s_count[kCcBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool ok = true;
    uint32_t roots = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanPerThread; j++) {
        const uint32_t cell = blockIdx.x * kScanCells + j * kCcBlock + threadIdx.x;
        bool is_root = false;
        if (cell < n) {
            int32_t r = g_load(&parent[cell]);
            if (r >= 0) {
                r = g_find(parent, r, n + 1, ok);
                atomicMin(&parent[cell], r);
                is_root = r == (int32_t)cell;
            }
            labels[cell] = r;
        }
        uint32_t in_wave;
        flags_below(is_root, lane, in_wave);
        roots += in_wave;
    }
    if (lane == 0) s_count[wave] = roots;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < kCcBlock / 64; w++) total += s_count[w];
        sums[blockIdx.x] = total;
    }
    if (!ok) cc_fail(err, kStageFlatten);
}

// ---- stage 4: the exclusive prefix sum of the block counts, one workgroup -------------------------------------------------------------
__global__ void __launch_bounds__(kScanBlock) k_cc_scan(uint32_t* __restrict__ sums, uint32_t n_blocks, const int32_t* __restrict__ err,
                                                        int32_t* __restrict__ n_components) {
    __shared__ uint32_t s_wave[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += kScanBlock) {      // (uniform trip count: every lane reaches the barriers)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? sums[i] : 0;
        const uint32_t inc = scan_inclusive<AddOp>(v, lane);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kScanBlock / 64; w++) {
            const uint32_t c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (i < n_blocks) sums[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int32_t e = *err;
        *n_components = e ? -e : (int32_t)carry;
    }
}

// ---- stage 5: roots take their rank (in `parent`, which nothing reads in this launch) -------------------------------------------------
__global__ void __launch_bounds__(kCcBlock) k_cc_rank(uint32_t n, const int32_t* __restrict__ labels, const uint32_t* __restrict__ sums,
                                                      int32_t* __restrict__ parent) {
    __shared__ uint32_t s_count[kScanPerThread][kCcBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool is_root[kScanPerThread];
    uint32_t below[kScanPerThread];
#pragma unroll
    for (uint32_t j = 0; j < kScanPerThread; j++) {
        const uint32_t cell = blockIdx.x * kScanCells + j * kCcBlock + threadIdx.x;
        is_root[j] = cell < n && labels[cell] == (int32_t)cell;
        uint32_t in_wave;
        below[j] = flags_below(is_root[j], lane, in_wave);
        if (lane == 0) s_count[j][wave] = in_wave;
    }
    __syncthreads();
    const uint32_t first = sums[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < kScanPerThread; j++) {
        if (!is_root[j]) continue;
        uint32_t before = 0;
        for (uint32_t q = 0; q < kScanPerThread * (kCcBlock / 64); q++)
            before += q < j * (kCcBlock / 64) + wave ? s_count[q / (kCcBlock / 64)][q % (kCcBlock / 64)] : 0;
        parent[blockIdx.x * kScanCells + j * kCcBlock + threadIdx.x] = (int32_t)(1 + first + before + below[j]);
    }
}

// ---- stage 6 -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcBlock) k_cc_relabel(uint32_t n, const int32_t* __restrict__ parent, int32_t* __restrict__ labels) {
    const uint32_t cell = blockIdx.x * kCcBlock + threadIdx.x;
    if (cell >= n) return;
    const int32_t r = labels[cell];
    labels[cell] = r >= 0 ? parent[r] : 0;
}

// ---- per-component statistics ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCcBlock) k_cc_stats_init(uint32_t n, int64_t* __restrict__ cells, int32_t* __restrict__ lo, int32_t* __restrict__ hi,
                                                            int64_t* __restrict__ overlap) {
    const uint32_t c = blockIdx.x * kCcBlock + threadIdx.x;
    if (c >= n) return;
    cells[c] = 0;
    if (overlap) overlap[c] = 0;
    for (int d = 0; d < 3; d++) {
        lo[3 * c + d] = INT_MAX;
        hi[3 * c + d] = -1;
    }
}

template <bool kMin>
__device__ __forceinline__ int wave_minmax(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int u = __shfl_xor(v, off, 64);
        v = kMin ? min(v, u) : max(v, u);
    }
    return v;
}

// what a wave has gathered for ONE label and not yet added to the tables: the same values in every lane
struct StatsRun {
    int32_t label;          // 0: nothing held
    uint32_t cells, marked;
    int lx, ly, lz, hx, hy, hz;
};

__device__ __forceinline__ void stats_flush(const StatsRun& r, uint32_t lane, int64_t* cells, int32_t* lo, int32_t* hi, int64_t* overlap) {
    if (r.label == 0 || lane != 0) return;
    const size_t c = (size_t)(r.label - 1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&cells[c]), (unsigned long long)r.cells);
    if (overlap && r.marked) atomicAdd(reinterpret_cast<unsigned long long*>(&overlap[c]), (unsigned long long)r.marked);
    atomicMin(&lo[3 * c + 0], r.lx);
    atomicMin(&lo[3 * c + 1], r.ly);
    atomicMin(&lo[3 * c + 2], r.lz);
    atomicMax(&hi[3 * c + 0], r.hx);
    atomicMax(&hi[3 * c + 1], r.hy);
    atomicMax(&hi[3 * c + 2], r.hz);
}

// A wave walks kStatsChunks consecutive chunks of 64 cells.  Per chunk, the lanes of every distinct label are reduced in the wave; the
// result joins the run the wave holds when it is of the same label, else the held run goes to the tables and this one is held.  A large
// component therefore costs one set of atomics per wave (64 * kStatsChunks cells), a map of small pieces one per piece and chunk.
__global__ void __launch_bounds__(kCcBlock) k_cc_stats(const int32_t* __restrict__ labels, uint32_t Y, uint32_t Z, uint32_t n_cells, int32_t n,
                                                       const uint8_t* __restrict__ truth, int64_t* cells, int32_t* lo, int32_t* hi, int64_t* overlap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t first = (blockIdx.x * (kCcBlock / 64) + (threadIdx.x >> 6)) * (64 * kStatsChunks);      // (< n_cells + 2^18: no overflow)
    StatsRun run = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < kStatsChunks; j++) {
        if (first + j * 64 >= n_cells) break;          // (the same in every lane of the wave)
        const uint32_t cell = first + j * 64 + lane;
        int32_t label = 0;
        if (cell < n_cells) label = labels[cell];
        if (label < 0 || label > n) label = 0;          // (labels of another n: never index past the tables)
        const int z = (int)(cell % Z), y = (int)((cell / Z) % Y), x = (int)(cell / (Z * Y));
        const bool marked = label != 0 && truth != nullptr && truth[cell] != 0;
        uint64_t todo = __ballot(label != 0);
        for (int round = 0; round < 64 && todo; round++) {      // at most 64 distinct labels in a wave
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int32_t cur = __shfl(label, leader, 64);
            const bool same = label == cur;
            const uint64_t group = __ballot(same);
            todo &= ~group;
            StatsRun g;
            g.label = cur;
            g.cells = (uint32_t)__popcll(group);
            g.marked = (uint32_t)__popcll(__ballot(same && marked));
            g.lx = wave_minmax<true>(same ? x : INT_MAX), g.ly = wave_minmax<true>(same ? y : INT_MAX), g.lz = wave_minmax<true>(same ? z : INT_MAX);
            g.hx = wave_minmax<false>(same ? x : -1), g.hy = wave_minmax<false>(same ? y : -1), g.hz = wave_minmax<false>(same ? z : -1);
            if (cur == run.label) {
                run.cells += g.cells, run.marked += g.marked;
                run.lx = min(run.lx, g.lx), run.ly = min(run.ly, g.ly), run.lz = min(run.lz, g.lz);
                run.hx = max(run.hx, g.hx), run.hy = max(run.hy, g.hy), run.hz = max(run.hz, g.hz);
            } else {
                stats_flush(run, lane, cells, lo, hi, overlap);
                run = g;
            }
        }
    }
    stats_flush(run, lane, cells, lo, hi, overlap);
}

static bool cc_size_ok(uint32_t X, uint32_t Y, uint32_t Z) {
    return X >= 1 && Y >= 1 && Z >= 1 && (uint64_t)X * Y < ((uint64_t)1 << 31) && (uint64_t)X * Y * Z < ((uint64_t)1 << 31);
}
constexpr size_t kCcHeader = 64;      // the error word, padded

struct CcWs {
    int32_t *err, *parent;      // the error word; [n] the union-find forest, later the ranks
    uint32_t* sums;             // [scan_blocks] roots per block of kScanCells cells
    uint32_t scan_blocks;
};
static CcWs cc_layout(Carver& c, uint32_t n) {
    CcWs w;
    w.scan_blocks = div_up(n, kScanCells);
    w.err = c.take<int32_t>(1);
    c.pad(kCcHeader - sizeof(int32_t));      // keeps `parent` on a 64-byte line of its own; no kernel touches it
    w.parent = c.take<int32_t>(n);
    w.sums = c.take<uint32_t>(w.scan_blocks);
    return w;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_label_components_workspace(uint32_t X, uint32_t Y, uint32_t Z) {
    if (!cc_size_ok(X, Y, Z)) return 0;
    Carver c; cc_layout(c, X * Y * Z); return c.bytes();
}

int ngp_label_components(const uint8_t* occupied, uint32_t X, uint32_t Y, uint32_t Z, uint32_t connectivity, int32_t* labels,
                         int32_t* n_components, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    NGP_REQUIRE(cc_size_ok(X, Y, Z), "label_components: every dimension >= 1 and X * Y * Z < 2^31 (got %u x %u x %u)", X, Y, Z);
    const uint32_t fwd = forward_mask(connectivity);
    NGP_REQUIRE(fwd != 0, "label_components: connectivity is 6, 14, 18 or 26 (got %u)", connectivity);
    NGP_REQUIRE(occupied && labels && n_components, "label_components: null pointer");
    int rc = check_workspace("label_components", workspace, workspace_bytes, ngp_label_components_workspace(X, Y, Z), 4);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = X * Y * Z;
    Carver c(workspace);
    const CcWs w = cc_layout(c, n);
    int32_t *const err = w.err, *const parent = w.parent;
    const uint32_t tiles_x = div_up(X, kTX), tiles_y = div_up(Y, kTY), tiles_z = div_up(Z, kTZ);
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y * tiles_z;
    NGP_REQUIRE(tiles < ((uint64_t)1 << 31), "label_components: %llu tiles of %u x %u x %u cells do not fit one launch", (unsigned long long)tiles,
                kTX, kTY, kTZ);
    const uint32_t cell_blocks = div_up(n, kCcBlock), scan_blocks = w.scan_blocks;
    if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return check_launch("label_components");
    {
        ProfScope prof("cc_tile", s, (double)n);
        k_cc_tile<<<(uint32_t)tiles, kTileCells, 0, s>>>(occupied, X, Y, Z, tiles_y, tiles_z, fwd, parent, err);
    }
    {
        ProfScope prof("cc_seams", s, (double)n);
        k_cc_seams<<<cell_blocks, kCcBlock, 0, s>>>(occupied, X, Y, Z, n, fwd, parent, err);
    }
    {
        ProfScope prof("cc_flatten", s, (double)n);
        k_cc_flatten<<<scan_blocks, kCcBlock, 0, s>>>(n, parent, labels, w.sums, err);
    }
    {
        ProfScope prof("cc_rank", s, (double)n);
        k_cc_scan<<<1, kScanBlock, 0, s>>>(w.sums, scan_blocks, err, n_components);
        k_cc_rank<<<scan_blocks, kCcBlock, 0, s>>>(n, labels, w.sums, parent);
        k_cc_relabel<<<cell_blocks, kCcBlock, 0, s>>>(n, parent, labels);
    }
    return check_launch("label_components");
}

int ngp_component_stats(const int32_t* labels, uint32_t X, uint32_t Y, uint32_t Z, int32_t n, const uint8_t* truth, int64_t* cells, int32_t* lo,
                        int32_t* hi, int64_t* overlap, ngp_stream_t stream) {
    if (n < 0 && n >= -(int32_t)kStageFlatten) {
        set_error("label_components: a loop reached its bound in stage '%s' (n_components = %d): the labels are not valid", kStageName[-n], n);
        return NGP_ELAUNCH;
    }
    NGP_REQUIRE(n >= 0, "component_stats: n >= 0 (got %d)", n);
    NGP_REQUIRE(cc_size_ok(X, Y, Z), "component_stats: every dimension >= 1 and X * Y * Z < 2^31 (got %u x %u x %u)", X, Y, Z);
    if (n == 0) return NGP_OK;
    NGP_REQUIRE(labels && cells && lo && hi, "component_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n_cells = X * Y * Z;
    ProfScope prof("cc_stats", s, (double)n_cells);
    k_cc_stats_init<<<div_up((uint32_t)n, kCcBlock), kCcBlock, 0, s>>>((uint32_t)n, cells, lo, hi, overlap);
    k_cc_stats<<<div_up(n_cells, kCcBlock * kStatsChunks), kCcBlock, 0, s>>>(labels, Y, Z, n_cells, n, truth, cells, lo, hi, overlap);
    return check_launch("component_stats");
}

}  // extern "C"
