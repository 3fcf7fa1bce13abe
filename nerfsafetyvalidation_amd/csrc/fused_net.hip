// fused_net.hip -- the one definition of what fused_net.hpp declares for the host, and the kernels that are not templates over a
// call site: packing FFMLP-layout weight blobs into MFMA fragment order (forward and transposed, fp16 and fp32), the per-cell corner
// records of the hash grid's dense levels, and the diagnostics (ngp_debug_*: fused features, stamps, sample hash, gradient dump).
// The network these serve is nerf/network_ff.py / nerf/network.py; the fragment orders are documented in fused_net.hpp.
#include <mutex>

#include "fused_net.hpp"

namespace ngp {

__global__ void k_pack_weights(const _Float16* __restrict__ sig, uint32_t sig_mm, const _Float16* __restrict__ col, uint32_t col_mm,
                               _Float16* __restrict__ packed) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_sig = sig_halfs(sig_mm), n_col = sig_halfs(col_mm);
    if (e >= n_sig + n_col) return;
    const bool is_col = e >= n_sig;
    const uint32_t r = is_col ? e - n_sig : e;
    const uint32_t mm = is_col ? col_mm : sig_mm;
    const _Float16* src = is_col ? col : sig;
    const uint32_t j = r & 7, lane = (r >> 3) & 63, c = lane & 15, q = lane >> 4;
    uint32_t src_idx;
    if (r < 2048) {                                   // input layer [ob][lane][8]
        const uint32_t ob = r >> 9;
        const uint32_t k = is_col ? perm_color(q, j) : perm_grid(q, j);
        src_idx = (16 * ob + c) * 32 + k;
    } else if (r < 2048 + mm * 4096) {                // hidden layers [k][ob][s][lane][8]
        const uint32_t rr = r - 2048, layer = rr >> 12, in = rr & 4095;
        const uint32_t ob = in >> 10, s = (in >> 9) & 1;
        src_idx = 2048 + layer * 4096 + (16 * ob + c) * 64 + perm_hidden(q, j, s);
    } else {                                          // output layer [s][lane][8]
        const uint32_t in = r - 2048 - mm * 4096, s = in >> 9;
        src_idx = 2048 + mm * 4096 + c * 64 + perm_hidden(q, j, s);
    }
    packed[e] = src[src_idx];
}

__global__ void k_pack_weights_f32(const float* __restrict__ sig, uint32_t sig_mm, const float* __restrict__ col, uint32_t col_mm,
                                   float* __restrict__ packed) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_sig = sig_halfs(sig_mm), n_col = sig_halfs(col_mm);
    if (e >= n_sig + n_col) return;
    const bool is_col = e >= n_sig;
    const uint32_t r = is_col ? e - n_sig : e;
    const uint32_t mm = is_col ? col_mm : sig_mm;
    const float* src = is_col ? col : sig;
    const uint32_t r4 = r & 3, lane = (r >> 2) & 63, c = lane & 15, q = lane >> 4;
    uint32_t src_idx;
    if (r < 2048) {                                   // input layer [ob][g][lane][4]
        const uint32_t blk = r >> 8, ob = blk >> 1, g = blk & 1, j = 4 * g + r4;
        src_idx = (16 * ob + c) * 32 + (is_col ? perm_color(q, j) : perm_grid(q, j));
    } else if (r < 2048 + mm * 4096) {                // hidden layers [k][ob][g][lane][4]
        const uint32_t rr = r - 2048, layer = rr >> 12, blk = (rr & 4095) >> 8, ob = blk >> 2, g = blk & 3;
        src_idx = 2048 + layer * 4096 + (16 * ob + c) * 64 + 16 * g + 4 * q + r4;
    } else {                                          // output layer [g][lane][4]
        const uint32_t g = (r - 2048 - mm * 4096) >> 8;
        src_idx = 2048 + mm * 4096 + c * 64 + 16 * g + 4 * q + r4;
    }
    packed[e] = src[src_idx];
}

__global__ void k_pack_weights_bwd_f32(const float* __restrict__ sig, uint32_t sig_mm, const float* __restrict__ col, uint32_t col_mm,
                                       float* __restrict__ packed) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_sig = bwd_floats(sig_mm), n_col = bwd_floats(col_mm);
    if (e >= n_sig + n_col) return;
    const bool is_col = e >= n_sig;
    const uint32_t r = is_col ? e - n_sig : e;
    const uint32_t mm = is_col ? col_mm : sig_mm;
    const float* src = is_col ? col : sig;
    const uint32_t r4 = r & 3, lane = (r >> 2) & 63, c = lane & 15, q = lane >> 4;
    const uint32_t w_hid = 2048, w_out = 2048 + mm * 4096;
    float v;
    if (r < 1024) {                                                   // out layer [ob][lane][4]
        const uint32_t ob = r >> 8;
        v = src[w_out + (4 * q + r4) * 64 + 16 * ob + c];
    } else if (r < 1024 + mm * 4096) {                                // hidden layers, last first
        const uint32_t rr = r - 1024, slot = rr >> 12, blk = (rr & 4095) >> 8, ob = blk >> 2, g = blk & 3;
        const uint32_t layer = mm - 1 - slot;
        v = src[w_hid + layer * 4096 + (16 * g + 4 * q + r4) * 64 + 16 * ob + c];
    } else {                                                          // in layer [ob 2][g 4][lane][4]
        const uint32_t blk = (r - 1024 - mm * 4096) >> 8, ob = blk >> 2, g = blk & 3;
        const uint32_t qq = c >> 2, jj = 4 * ob + (c & 3);
        v = src[(16 * g + 4 * q + r4) * 32 + (is_col ? perm_color(qq, jj) : perm_grid(qq, jj))];
    }
    packed[e] = v;
}

__global__ void k_pack_weights_bwd(const _Float16* __restrict__ sig, uint32_t sig_mm, const _Float16* __restrict__ col, uint32_t col_mm,
                                   _Float16* __restrict__ packed) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_sig = bwd_halfs(sig_mm), n_col = bwd_halfs(col_mm);
    if (e >= n_sig + n_col) return;
    const bool is_col = e >= n_sig;
    const uint32_t r = is_col ? e - n_sig : e;
    const uint32_t mm = is_col ? col_mm : sig_mm;
    const _Float16* src = is_col ? col : sig;
    const uint32_t j = r & 7, lane = (r >> 3) & 63, c = lane & 15, q = lane >> 4;
    const uint32_t w_hid = 2048, w_out = 2048 + mm * 4096;           // offsets inside the FFMLP-layout source blob
    _Float16 v;
    if (r < 2048) {                                                   // out layer [ob][lane][8]
        const uint32_t ob = r >> 9;
        v = j < 4 ? src[w_out + (4 * q + j) * 64 + 16 * ob + c] : (_Float16)0;
    } else if (r < 2048 + mm * 4096) {                                // hidden layers, last first
        const uint32_t rr = r - 2048, slot = rr >> 12, in = rr & 4095;
        const uint32_t layer = mm - 1 - slot;
        const uint32_t ob = in >> 10, st = (in >> 9) & 1;
        v = src[w_hid + layer * 4096 + perm_hidden(q, j, st) * 64 + 16 * ob + c];
    } else {                                                          // in layer [ob 2][s 2][lane][8]
        const uint32_t in = r - 2048 - mm * 4096, ob = in >> 10, st = (in >> 9) & 1;
        const uint32_t i = c, qq = i >> 2, jj = 4 * ob + (i & 3);
        const uint32_t feat = is_col ? perm_color(qq, jj) : perm_grid(qq, jj);
        v = src[perm_hidden(q, j, st) * 32 + feat];
    }
    packed[e] = v;
}

// Diagnostics: the 32 hash-grid features as the fused kernels form them ([M, 32] fp16 in the operator's order 2 * level + channel),
// with the default arithmetic or with the operator's (HALF_ACC)
template <int MODE, bool HALF_ACC>
__global__ void __launch_bounds__(256) k_debug_features(NetArgs na, GridLevels lv, const float* __restrict__ xyzs, uint32_t M, _Float16* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* Wlds = reinterpret_cast<_Float16*>(smem);
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + net_w_bytes_f16(na));
    stage_block(na, lv, Wlds, lt, net_w_bytes_f16(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t tile = wave; tile < (M + 15) / 16; tile += n_waves) {
        const uint32_t m = tile * 16 + c, mm = m < M ? m : M - 1;
        uint32_t raw[4][8];
        float fr[4][3];
        bool oob;
        fused_gather<MODE>(na, *lt, q, xyzs[(size_t)mm * 3], xyzs[(size_t)mm * 3 + 1], xyzs[(size_t)mm * 3 + 2], raw, fr, oob);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            _Float16 f0, f1;
            corners_to_feature<HALF_ACC>(fr[i], raw[i], oob, f0, f1);
            if (m < M) { out[(size_t)m * 32 + 2 * (q + 4 * i)] = f0; out[(size_t)m * 32 + 2 * (q + 4 * i) + 1] = f1; }
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) k_debug_features32(NetArgs na, GridLevels lv, const float* __restrict__ xyzs, uint32_t M, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + net_w_bytes(na));
    stage_block(na, lv, smem, lt, net_w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t tile = wave; tile < (M + 15) / 16; tile += n_waves) {
        const uint32_t m = tile * 16 + c, mm = m < M ? m : M - 1;
        float feat[8];
        NetF32<MODE>::features(na, *lt, q, xyzs[(size_t)mm * 3], xyzs[(size_t)mm * 3 + 1], xyzs[(size_t)mm * 3 + 2], feat);
        if (m < M) {
#pragma unroll
            for (int i = 0; i < 4; i++) { out[(size_t)m * 32 + 2 * (q + 4 * i)] = feat[2 * i]; out[(size_t)m * 32 + 2 * (q + 4 * i) + 1] = feat[2 * i + 1]; }
        }
    }
}

static std::mutex g_debug_mu;
static DebugState g_debug_default;
static float* g_grad_dump = nullptr;     // ngp_debug_set_grad_dump

DebugState debug_snapshot() {
    std::lock_guard<std::mutex> lk(g_debug_mu);
    return g_debug_default;
}

bool debug_flags_valid(int flags, const char* who) {
    if ((flags & ~NGP_DBG_ALL) == 0) return true;
    set_error("%s: unknown debug flag bits 0x%x (the NGP_DBG_* constants are all there are)", who, (unsigned)(flags & ~NGP_DBG_ALL));
    return false;
}

float* grad_dump() { return g_grad_dump; }

// records needed for the first n_levels levels (0 when they do not fit 32-bit record indices)
static uint64_t cell_records(const GridLevels& lv, uint32_t n_levels, uint32_t* off) {
    uint64_t total = 0;
    for (uint32_t l = 0; l < n_levels; l++) {
        if (off) off[l] = (uint32_t)total;
        const uint64_t S = lv.resolution[l];
        total += S * S * S;
    }
    return total < (1ull << 32) ? total : 0;
}

bool needs_generic(const GridLevels& lv) {
    for (int l = 0; l < 16; l++)
        if (lv.mode[l] == 2) return true;
    return false;
}

int fill_net(const ngp_model* m, const _Float16* packed, NetArgs& na, GridLevels& lv) {
    NGP_REQUIRE(m && m->embeddings && m->offsets_host && m->sigma_weights && m->color_weights, "ngp_model: null pointer");
    NGP_REQUIRE(m->L == 16, "fused renderer: the hash grid must have 16 levels with 2 features (got L=%u)", m->L);
    NGP_REQUIRE(m->sigma_hidden_mm <= 2 && m->color_hidden_mm <= 3, "fused renderer: at most 2 / 3 hidden matmuls (got %u / %u)",
                m->sigma_hidden_mm, m->color_hidden_mm);
    fill_levels(lv, m->offsets_host, 16, m->S, m->H_base, 3, m->gridtype, m->align_corners != 0);
    na.table = reinterpret_cast<const uint32_t*>(m->embeddings);
    na.packed = packed;
    na.sig_mm = m->sigma_hidden_mm;
    na.col_mm = m->color_hidden_mm;
    na.bound = m->bound;
    na.inv_two_bound = 1.0f / (2 * m->bound);
    na.density_scale = m->density_scale;
    na.align_corners = m->align_corners;
    NGP_REQUIRE(m->precision <= NGP_PREC_F16_REF, "ngp_model: unknown precision %u", m->precision);
    na.prec_bits = (m->precision == NGP_PREC_F32 ? 256u : 0u) | (m->precision == NGP_PREC_F16_REF ? 512u : 0u);
    // the fused gathers address the table with a 32-bit byte offset (table_at)
    NGP_REQUIRE((uint64_t)m->offsets_host[16] * (na.f32() ? 8u : 4u) < (1ull << 32), "fused renderer: the hash table must be smaller than 4 GiB (%u entries)",
                (unsigned)m->offsets_host[16]);
    na.cells = nullptr;
    na.cell_steps = 0;
    for (int l = 0; l < 16; l++) na.cell_off[l] = 0;
    if (m->cell_tables && m->cell_levels) {
        NGP_REQUIRE(m->cell_levels % 4 == 0 && m->cell_levels <= 16, "ngp_model: cell_levels must be 0, 4, 8, 12 or 16 (got %u)", m->cell_levels);
        NGP_REQUIRE(cell_records(lv, m->cell_levels, na.cell_off) != 0, "ngp_model: the cell tables of %u levels exceed 2^32 records", m->cell_levels);
        NGP_REQUIRE(((uintptr_t)m->cell_tables & 15) == 0, "ngp_model: cell_tables must be 16-byte aligned");
        NGP_REQUIRE(!na.f32(), "ngp_model: per-cell records exist for the fp16 table only");
        if (m->cell_levels == 12 && !needs_generic(lv)) {   // the kernels are specialised for exactly 12 expanded levels
            na.cells = reinterpret_cast<const uint4*>(m->cell_tables);
            na.cell_steps = 3;
        }
    }
    return NGP_OK;
}

size_t weights_bytes(const NetArgs& na) { return net_w_bytes(na); }
// Workgroups of a grid-strided launch: as many as are RESIDENT at once -- four 256-thread workgroups per CU, or what the LDS holds (the
// fp32 weights take 40 KB per workgroup: three).  With more, the surplus of every CU runs as a second round at a fraction of the occupancy.
uint32_t resident_blocks(size_t lds) {
    const uint32_t fit = (uint32_t)((160 * 1024) / (lds ? lds : 1));
    return 256u * (fit > 4 ? 4u : (fit < 1 ? 1u : fit));
}

// kernel variant of a model: 0 / 1 / 2 = fp16 (AND-reduced indices, generic modulo, per-cell records), 3 / 4 = fp32 (AND, generic),
// 5 / 6 / 7 = fp16 with the reference's corner rounding
int net_variant(const NetArgs& na, const GridLevels& lv) {
    const bool gen = needs_generic(lv);
    if (na.f32()) return gen ? 4 : 3;
    return (gen ? 1 : (na.cells ? 2 : 0)) + (na.hacc() ? 5 : 0);
}

// 2*bound = 2^k: then (x + bound) * inv_two_bound maps [-bound, bound] onto [0, 1] exactly (inv_two_bound is the exact reciprocal)
// and a kernel that clamps its positions may drop the encoder's out-of-range test (encoder_unit<CLAMPED>)
bool clamped_exact(const NetArgs& na) {
    int e = 0;
    return na.bound > 0.0f && std::isfinite(na.bound) && frexpf(na.bound, &e) == 0.5f && na.inv_two_bound * (2 * na.bound) == 1.0f;
}

// the fp32 backward kernels keep at most 1 / 2 hidden layers' activations (NetF32::Tape; nerf/network.py has 0 / 1)
bool bwd_shape_ok(const NetArgs& na) { return !na.f32() || (na.sig_mm <= NetF32<0>::kMaxSigMM && na.col_mm <= NetF32<0>::kMaxColMM); }

}  // namespace ngp

using namespace ngp;

// per-cell corner records: record r of level l (cells x-fastest, `res` per axis) = the table entries of the cell's 8 corners in
// the gather's corner order (bit 0 of the corner index = x).  One thread per record.  (Deliberately outside namespace ngp: an unqualified symbol.)
__global__ void __launch_bounds__(256) k_build_cells(const uint32_t* __restrict__ table, GridLevels lv, uint32_t level, uint32_t n_cells,
                                                     uint4* __restrict__ out) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_cells) return;
    const uint32_t S = lv.resolution[level];
    const uint32_t cx = r % S, cy = (r / S) % S, cz = r / (S * S);
    const uint32_t size = lv.offset[level + 1] - lv.offset[level];
    const bool hashed = lv.hashed[level] != 0;
    const uint32_t a1 = hashed ? 2654435761u : lv.mul1[level], a2 = hashed ? 805459861u : lv.mul2[level];
    const uint32_t* tab = table + lv.offset[level];
    uint32_t v[8];
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
        const uint32_t px = cx + (idx & 1), ty = (cy + ((idx >> 1) & 1)) * a1, tz = (cz + ((idx >> 2) & 1)) * a2;
        uint32_t e = hashed ? (px ^ ty ^ tz) : (px + ty + tz);
        if (lv.mode[level] == 1) e &= size - 1;
        else if (lv.mode[level] == 2) e %= size;
        v[idx] = tab[e];
    }
    out[(size_t)r * 2] = make_uint4(v[0], v[1], v[2], v[3]);
    out[(size_t)r * 2 + 1] = make_uint4(v[4], v[5], v[6], v[7]);
}

extern "C" {

size_t ngp_cell_tables_bytes(const ngp_model* model, uint32_t n_levels) {
    if (!model || !model->offsets_host || model->L != 16 || n_levels > 16) return 0;
    GridLevels lv;
    fill_levels(lv, model->offsets_host, 16, model->S, model->H_base, 3, model->gridtype, model->align_corners != 0);
    return (size_t)cell_records(lv, n_levels, nullptr) * 32;
}

int ngp_build_cell_tables(const ngp_model* model, uint32_t n_levels, void* out, ngp_stream_t stream) {
    NGP_REQUIRE(model && model->embeddings && model->offsets_host && out, "build_cell_tables: null pointer");
    NGP_REQUIRE(model->L == 16 && n_levels % 4 == 0 && n_levels >= 4 && n_levels <= 16, "build_cell_tables: n_levels must be 4, 8, 12 or 16");
    NGP_REQUIRE(((uintptr_t)out & 15) == 0, "build_cell_tables: the buffer must be 16-byte aligned");
    GridLevels lv;
    fill_levels(lv, model->offsets_host, 16, model->S, model->H_base, 3, model->gridtype, model->align_corners != 0);
    uint32_t off[16];
    NGP_REQUIRE(cell_records(lv, n_levels, off) != 0, "build_cell_tables: %u levels exceed 2^32 records", n_levels);
    for (uint32_t l = 0; l < n_levels; l++) {
        const uint64_t S = lv.resolution[l];
        const uint32_t n = (uint32_t)(S * S * S);
        k_build_cells<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const uint32_t*>(model->embeddings), lv, l, n,
                                                                       reinterpret_cast<uint4*>(out) + (size_t)off[l] * 2);
    }
    return check_launch("build_cell_tables");
}

int ngp_debug_set_stamps(unsigned long long* device_buf) {
    std::lock_guard<std::mutex> lk(g_debug_mu);
    g_debug_default.stamps = device_buf;
    return NGP_OK;
}

int ngp_debug_set_sample_hash(uint32_t* device_buf) {
    std::lock_guard<std::mutex> lk(g_debug_mu);
    g_debug_default.sample_hash = device_buf;
    return NGP_OK;
}

int ngp_debug_disable_march_queue(int flags) {
    if (!debug_flags_valid(flags, "debug_disable_march_queue")) return NGP_EINVAL;
    std::lock_guard<std::mutex> lk(g_debug_mu);
    g_debug_default.flags = flags;
    return NGP_OK;
}

int ngp_debug_fused_features(const ngp_model* model, const float* xyzs, uint32_t M, int operator_rounding, uint16_t* features, ngp_stream_t stream) {
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyzs && features, "debug_fused_features: null pointer");
    NGP_REQUIRE(model && model->packed_weights, "debug_fused_features: model->packed_weights is NULL (ngp_pack_weights fills it)");
    hipStream_t s = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    const size_t lds = weights_bytes(na) + sizeof(LevelTab);
    uint32_t blocks = div_up(div_up(M, 16), 4);
    if (blocks > resident_blocks(lds)) blocks = resident_blocks(lds);
    if (na.f32()) {   // `features` is float [M, 32] then; one arithmetic only (the operator's)
        if (needs_generic(lv)) k_debug_features32<1><<<blocks, 256, lds, s>>>(na, lv, xyzs, M, (float*)features);
        else k_debug_features32<0><<<blocks, 256, lds, s>>>(na, lv, xyzs, M, (float*)features);
        return check_launch("debug_fused_features");
    }
    const int mode = needs_generic(lv) ? 1 : (na.cells ? 2 : 0);
#define NGP_DBG_FEAT(MODE_, HA_)                                                                              \
    ensure_dynamic_lds(reinterpret_cast<const void*>(k_debug_features<MODE_, HA_>), 96 * 1024);               \
    k_debug_features<MODE_, HA_><<<blocks, 256, lds, s>>>(na, lv, xyzs, M, (_Float16*)features)
    if (operator_rounding) {
        if (mode == 1) { NGP_DBG_FEAT(1, true); } else if (mode == 2) { NGP_DBG_FEAT(2, true); } else { NGP_DBG_FEAT(0, true); }
    } else {
        if (mode == 1) { NGP_DBG_FEAT(1, false); } else if (mode == 2) { NGP_DBG_FEAT(2, false); } else { NGP_DBG_FEAT(0, false); }
    }
#undef NGP_DBG_FEAT
    return check_launch("debug_fused_features");
}

int ngp_debug_set_grad_dump(float* device_buf) {
    g_grad_dump = device_buf;
    return NGP_OK;
}

size_t ngp_packed_weights_bytes(void) { return (size_t)(sig_halfs(2) + sig_halfs(3)) * 4; }   // (sized for the fp32 form; fp16 uses half of it)

int ngp_pack_weights(const ngp_model* model, void* out, ngp_stream_t stream) {
    NGP_REQUIRE(model && model->sigma_weights && model->color_weights && out, "pack_weights: null pointer");
    NGP_REQUIRE(model->sigma_hidden_mm <= 2 && model->color_hidden_mm <= 3, "pack_weights: at most 2 / 3 hidden matmuls (got %u / %u)",
                model->sigma_hidden_mm, model->color_hidden_mm);
    NGP_REQUIRE(((uintptr_t)out & 15) == 0, "pack_weights: the buffer must be 16-byte aligned");
    const uint32_t n_packed = sig_halfs(model->sigma_hidden_mm) + sig_halfs(model->color_hidden_mm);
    if (model->precision == NGP_PREC_F32)
        k_pack_weights_f32<<<div_up(n_packed, 256), 256, 0, (hipStream_t)stream>>>((const float*)model->sigma_weights, model->sigma_hidden_mm,
                                                                                   (const float*)model->color_weights, model->color_hidden_mm,
                                                                                   (float*)out);
    else
        k_pack_weights<<<div_up(n_packed, 256), 256, 0, (hipStream_t)stream>>>((const _Float16*)model->sigma_weights, model->sigma_hidden_mm,
                                                                               (const _Float16*)model->color_weights, model->color_hidden_mm,
                                                                               (_Float16*)out);
    return check_launch("pack_weights");
}

size_t ngp_packed_weights_bwd_bytes(void) {      // (sized for whichever form is larger)
    const size_t h = (size_t)(bwd_halfs(2) + bwd_halfs(3)) * 2, f = (size_t)(bwd_floats(2) + bwd_floats(3)) * 4;
    return h > f ? h : f;
}

int ngp_pack_weights_bwd(const ngp_model* model, void* out, ngp_stream_t stream) {
    NGP_REQUIRE(model && model->sigma_weights && model->color_weights && out, "pack_weights_bwd: null pointer");
    NGP_REQUIRE(model->sigma_hidden_mm <= 2 && model->color_hidden_mm <= 3, "pack_weights_bwd: at most 2 / 3 hidden matmuls (got %u / %u)",
                model->sigma_hidden_mm, model->color_hidden_mm);
    NGP_REQUIRE(((uintptr_t)out & 15) == 0, "pack_weights_bwd: the buffer must be 16-byte aligned");
    if (model->precision == NGP_PREC_F32) {
        const uint32_t n = bwd_floats(model->sigma_hidden_mm) + bwd_floats(model->color_hidden_mm);
        k_pack_weights_bwd_f32<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>((const float*)model->sigma_weights, model->sigma_hidden_mm,
                                                                                (const float*)model->color_weights, model->color_hidden_mm, (float*)out);
    } else {
        const uint32_t n = bwd_halfs(model->sigma_hidden_mm) + bwd_halfs(model->color_hidden_mm);
        k_pack_weights_bwd<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>((const _Float16*)model->sigma_weights, model->sigma_hidden_mm,
                                                                            (const _Float16*)model->color_weights, model->color_hidden_mm, (_Float16*)out);
    }
    return check_launch("pack_weights_bwd");
}

}  // extern "C"
