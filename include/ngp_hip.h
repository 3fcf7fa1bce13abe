/*
 * ngp_hip.h -- C ABI of libngp_hip.so, the MI355X (gfx950) implementation of the
 * Instant-NGP render path of sisl/NeRFSafetyValidation.
 *
 * This is the drop-in boundary: one entry point per function of the reference's
 * four pybind11 extension modules (the only native interface its Python operator
 * layer calls), plus the fused MI355X-native render entry points that sit behind
 * nerf/renderer.py::NeRFRenderer.run_cuda.
 *
 *   reference interface replaced                          (file:line under /root/reference)
 *   _raymarching   raymarching/src/raymarching.h:7-18,    raymarching/src/bindings.cpp:5-18
 *   _gridencoder   gridencoder/src/gridencoder.h:12-13,   gridencoder/src/bindings.cpp:5-8
 *   _shencoder     shencoder/src/shencoder.h:10-13,       shencoder/src/bindings.cpp:5-8
 *   _ffmlp         ffmlp/src/ffmlp.h:8-15,                ffmlp/src/bindings.cpp:5-11
 *   _freqencoder   freqencoder/src/freqencoder.h:6-10,    freqencoder/src/bindings.cpp:5-8
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - the caller owns every buffer; nothing is allocated on the data path
 *     (scratch comes in through an explicit workspace argument);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream) and the call returns without synchronising, unless stated;
 *   - return value: 0 on success, a negative NGP_E* code otherwise;
 *     ngp_last_error() returns a thread-local description of the last failure.
 *     The reference raises c10::Error / std::runtime_error at the same places
 *     (gridencoder.cu:355,372,424-440; ffmlp.cu:636-658); the ctypes shim turns
 *     a non-zero return into RuntimeError;
 *   - dtype arguments: NGP_F32 or NGP_F16 (IEEE binary16).
 *   - argument ORDER follows the reference's native signatures, not the Python
 *     wrappers' (they differ: SURVEY.md section 8b).
 */
#ifndef NGP_HIP_H
#define NGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGP_OK 0
#define NGP_EINVAL (-1)    /* unsupported size / dtype / null pointer            */
#define NGP_ELAUNCH (-2)   /* hipGetLastError() after a launch                    */
#define NGP_EWORKSPACE (-3)/* workspace too small                                 */
#define NGP_ENODEVICE (-4) /* no HIP device                                       */

#define NGP_F32 0
#define NGP_F16 1

typedef void* ngp_stream_t;

#if defined(NGP_BUILD)
#define NGP_API __attribute__((visibility("default")))
#else
#define NGP_API
#endif

/* The number ngp_version() returns; it changes with every incompatible change of this header, and a binding compares it at load.
 *   101: ngp_network_density has a `geo_feat` argument, ngp_model has `precision` (both were added under 100, unrecorded).
 *   102: ngp_mark_untrained_grid_workspace is new; ngp_density_grid_update, ngp_density_grid_finish, ngp_uq_stats and
 *        ngp_mark_untrained_grid return NGP_EWORKSPACE, no longer NGP_EINVAL, for a workspace that is too small.
 *   103: ngp_box_mesh_overlap and ngp_box_cells_overlap are new.
 *   104: ngp_box_mesh_clearance and ngp_box_cells_clearance are new. */
#define NGP_ABI_VERSION 104

/* Caller-owned workspaces.  Every `workspace` / `workspace_bytes` pair below is checked by one rule, against the size its
 * ngp_*_workspace() function answers (which the entry point carves with the very code that measured it):
 *   nothing needed (the size function answers 0)                             -> not looked at, NULL is fine
 *   workspace_bytes smaller than needed (NULL with 0 bytes included)         -> NGP_EWORKSPACE, "<entry point>: workspace too small
 *                                                                               (<given> < <needed> bytes)" in ngp_last_error()
 *   enough bytes, but the pointer is NULL or not aligned as the entry states -> NGP_EINVAL
 * and nothing is launched in either case.  This holds for ngp_march_rays_train (16-byte aligned), ngp_edt_sq, ngp_label_components,
 * ngp_sift_interest_mask, ngp_mark_untrained_grid, ngp_photo_loss_forward, the ngp_distortion_* and ngp_depth_loss_* forwards
 * (4-byte), ngp_isosurface_count / _emit, ngp_distance_stats, ngp_density_grid_update / _finish, ngp_uq_stats, ngp_sigma_fit_* and
 * ngp_image_quality (8-byte).  Not for ngp_render_upsample, ngp_grid_encode_backward* and ngp_ffmlp_backward*, where the workspace
 * given chooses the route. */

NGP_API const char* ngp_last_error(void);
NGP_API int ngp_version(void);
/* number of HIP devices visible (does not create a context on this image) */
NGP_API int ngp_device_count(void);

/* ---------------- _raymarching (raymarching/src/raymarching.h:7-18) ---------------- */

/* raymarching.cu:150-158 near_far_from_aabb */
NGP_API int ngp_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near,
                           float* nears, float* fars, ngp_stream_t stream);
/* (this build) nerf/renderer.py:376-381 in one launch, in place: image [N,3] += (1 - weights_sum) * bg_color (three HOST floats),
 * depth [N] = clamp(depth - nears, min 0) / (fars - nears).  Same operations and roundings as the torch lines. */
NGP_API int ngp_finish_rays(float* image, float* depth, const float* weights_sum, const float* nears, const float* fars,
                    const float* bg_color3_host, uint32_t N, ngp_stream_t stream);
/* raymarching.cu:203-211 sph_from_ray */
NGP_API int ngp_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords,
                     ngp_stream_t stream);
/* raymarching.cu:231-234 / 259-262 */
NGP_API int ngp_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, ngp_stream_t stream);
NGP_API int ngp_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, ngp_stream_t stream);
/* raymarching.cu:294-302 packbits; N = number of output BYTES */
NGP_API int ngp_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, ngp_stream_t stream);

/* The occupancy grid of the marches below, of ngp_render_rays and of the density-grid maintenance: C cascades (1 <= C <= 8) of H^3
 * cells, cell (level, x, y, z) at bit level * H^3 + morton3D(x, y, z) of the bitfield, LSB first in a byte.  H must be a POWER OF TWO
 * in [2, 1024]: the Morton code of a cell stays below H^3 only then (H = 48: morton3D(47, 47, 47) = 233 471 against 110 592 cells), so
 * any other H would index past the level and past the buffer.  ngp_march_rays, ngp_march_rays_lin, ngp_march_rays_train,
 * ngp_render_rays, ngp_mark_untrained_grid, ngp_density_grid_update and ngp_density_grid_finish return NGP_EINVAL on the host for
 * anything else, name the sizes in ngp_last_error(), launch nothing and leave their outputs untouched. */

/* raymarching.cu:486-495 march_rays_train.  Slots are handed out by an exclusive
 * prefix sum in ray order (deterministic member of the reference's atomicAdd
 * permutation set).  counter[0] += total samples, counter[1] += N, as the
 * reference's atomics leave them.  workspace: ngp_march_rays_train_workspace(N) bytes, 16-byte aligned
 * (NGP_EWORKSPACE when smaller). */
NGP_API size_t ngp_march_rays_train_workspace(uint32_t N);
NGP_API int ngp_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                         uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                         const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                         uint32_t perturb, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
/* raymarching.cu:585-593 / 691-699 */
NGP_API int ngp_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                     uint32_t M, uint32_t N, float* weights_sum, float* depth, float* image,
                                     ngp_stream_t stream);
NGP_API int ngp_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                      const float* rgbs, const float* deltas, const int32_t* rays,
                                      const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                      float* grad_sigmas, float* grad_rgbs, ngp_stream_t stream);
/* raymarching.cu:817-825 march_rays.  The kernel itself zero-fills the unused tail of
 * every ray's n_step slots and rows [n_alive*n_step, M_padded) so the caller may pass
 * uninitialised buffers of M_padded rows (the reference wrapper passes torch.zeros). */
NGP_API int ngp_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                   uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars, float* xyzs,
                   float* dirs, float* deltas, uint32_t perturb, uint32_t M_padded, ngp_stream_t stream);
/* The same operator with derived copies of the occupancy bits held by the CALLER (built once per version of the bitfield: an x-fastest
 * re-layout and its one-bit-per-4x4x4-block reduction, as ngp_render_rays and ngp_march_rays_train keep them internally): cheaper probes,
 * one-step exits from empty blocks, no probe for the samples that follow in an occupied cell.  Same outputs bit for bit; 2-3 x the rate.
 * ngp_occupancy_lin_bytes: size of that buffer, 0 when the grid has none (H not a power of two, below 8, or too large);
 * ngp_build_occupancy_lin: fills it (grid 8-byte aligned, out 256-byte aligned) on `stream`. */
NGP_API size_t ngp_occupancy_lin_bytes(uint32_t C, uint32_t H);
NGP_API int ngp_build_occupancy_lin(const uint8_t* grid, uint32_t C, uint32_t H, void* out, size_t out_bytes, ngp_stream_t stream);
NGP_API int ngp_march_rays_lin(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                   uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars, float* xyzs,
                   float* dirs, float* deltas, uint32_t perturb, uint32_t M_padded, const void* occupancy_lin,
                   ngp_stream_t stream);
/* raymarching.cu:916-922 composite_rays (updates rays_alive, rays_t, weights_sum, depth, image in place) */
NGP_API int ngp_composite_rays(uint32_t n_alive, uint32_t n_step, int32_t* rays_alive, float* rays_t, const float* sigmas,
                       const float* rgbs, const float* deltas, float* weights_sum, float* depth, float* image,
                       ngp_stream_t stream);

/* ---------------- _gridencoder (gridencoder/src/gridencoder.h:12-13) ---------------- */

/* gridencoder.cu:415-446.  inputs f32 [B,D]; embeddings [sO,C] dtype; offsets_host: the
 * SAME int32[L+1] table as the device `offsets` tensor, in host memory (the level
 * geometry is evaluated on the host once per call); outputs [L,B,C] dtype;
 * dy_dx [B,L*D*C] dtype or NULL.  D in {2,3}, C in {1,2,4,8}.
 * cell_tables (optional, may be NULL; fp16, D = 3, C = 2 only): the per-cell corner records of the first cell_levels levels of
 * THIS table (ngp_build_cell_tables, below) -- a derived copy that turns eight 4-byte gathers per level into one 32-byte
 * record read.  Results are bit-identical with and without it; the caller rebuilds it when the table changes. */
NGP_API int ngp_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets_host, void* outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                            int calc_grad_inputs, void* dy_dx, uint32_t gridtype, int align_corners, int dtype,
                            const void* cell_tables, uint32_t cell_levels, ngp_stream_t stream);
/* gridencoder.cu:448-478.  grad [L,B,C]; grad_embeddings [sO,C] (accumulated into, caller zero-fills; NULL with calc_grad_inputs set = frozen table, only grad_inputs is produced);
 * grad_inputs [B,D] dtype or NULL. */
NGP_API int ngp_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings,
                             const int32_t* offsets_host, void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                             uint32_t L, float S, uint32_t H, int calc_grad_inputs, const void* dy_dx,
                             void* grad_inputs, uint32_t gridtype, int align_corners, int dtype, void* workspace,
                             size_t workspace_bytes, ngp_stream_t stream);
/* The same two operators with the position of a (level, point) feature group in outputs / grad given by the caller, in elements:
 * element (level, b, c) is at level * level_stride + b * point_stride + c.  (B * C, C) is the operator's [L,B,C]; (Bp * C, C) is level
 * planes with a padded row count Bp >= B -- what ngp_ffmlp_forward_planes / _backward_planes read and write in place, so that the
 * permute + copy of gridencoder/grid.py:52 and :72 (64 B read + 64 B written per point, each way) disappears; (C, L * C) is the
 * module's [B, L*C].  Same kernels, same arithmetic, same values; rows or planes the call does not address are left untouched. */
NGP_API int ngp_grid_encode_forward_strided(const float* inputs, const void* embeddings, const int32_t* offsets_host, void* outputs,
                                    uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                    int calc_grad_inputs, void* dy_dx, uint32_t gridtype, int align_corners, int dtype,
                                    const void* cell_tables, uint32_t cell_levels, uint32_t level_stride, uint32_t point_stride,
                                    ngp_stream_t stream);
NGP_API int ngp_grid_encode_backward_strided(const void* grad, const float* inputs, const void* embeddings,
                                     const int32_t* offsets_host, void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                                     uint32_t L, float S, uint32_t H, int calc_grad_inputs, const void* dy_dx,
                                     void* grad_inputs, uint32_t gridtype, int align_corners, int dtype, void* workspace,
                                     size_t workspace_bytes, uint32_t level_stride, uint32_t point_stride, ngp_stream_t stream);
/* The table gradient of large fp16 two-feature batches is a binned two-pass scatter through a CALLER-OWNED device workspace
 * (nothing is kept between calls, so calls on different streams are independent).  ngp_grid_encode_backward_workspace returns
 * the size that lets all levels go through the bins (0: this shape does not use one).  A smaller workspace makes the call process
 * the levels in smaller groups; NULL falls back to one atomic per update -- same result up to the order of the atomics. */
NGP_API size_t ngp_grid_encode_backward_workspace(uint32_t B, uint32_t D, uint32_t C, uint32_t L, int dtype);

/* ---------------- _shencoder (shencoder/src/shencoder.h:10-13) ---------------- */

/* shencoder.cu:402-420.  inputs f32 [B,3]; outputs f32 [B,C*C]; dy_dx f32 [B,3*C*C] or NULL; C = degree 1..8 */
NGP_API int ngp_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D, uint32_t C,
                          int calc_grad_inputs, float* dy_dx, ngp_stream_t stream);
/* shencoder.cu:422-441.  grad_inputs f32 [B,3] is ACCUMULATED into (caller zero-fills). */
NGP_API int ngp_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t C,
                           const float* dy_dx, float* grad_inputs, ngp_stream_t stream);

/* ---------------- _freqencoder (freqencoder/src/bindings.cpp:5-8) ---------------- */

/* freqencoder.cu:97-110.  inputs f32 [B,D]; outputs f32 [B,C], C = D + 2 D deg, columns
 *   [ x (D) | sin(2^0 x) (D) | cos(2^0 x) (D) | sin(2^1 x) (D) | cos(2^1 x) (D) | ... ]        (the reference's order, :28-58)
 * The first D columns are bit copies of the input; the others are full-precision sin / cos of the EXACT float 2^f x (within 4 ulp of
 * 1.0 of the real value; not the reference's __sinf(2^f x + pi/2)).  D >= 1, 0 <= deg <= 16 (0: the copy alone); B * C may pass 2^32
 * (64-bit indexing).  B = 0 succeeds without a launch. */
NGP_API int ngp_freq_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D, uint32_t deg, ngp_stream_t stream);
/* freqencoder.cu:113-129, but sin / cos are recomputed from `inputs` (the outputs are not read):
 *   grad_inputs[b,d] = grad[b,d] + sum_f 2^f (grad_sin[f,b,d] cos(2^f x) - grad_cos[f,b,d] sin(2^f x)),   f ascending, one thread
 * grad f32 [B,C]; grad_inputs f32 [B,D] is WRITTEN (no zero fill needed).  No atomics: the same bits on every call. */
NGP_API int ngp_freq_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t deg, float* grad_inputs,
                             ngp_stream_t stream);

/* ---------------- the elementwise steps between the two FFMLPs (nerf/network_ff.py:55-70) ----------------
 * What the reference's NeRFNetwork.forward does in torch between sigma_net and color_net, and after color_net, as one kernel each way
 * (values identical to the torch chain; host-side convenience of this build, the reference has no native entry for it):
 *   sigma [B] f32 = exp(float(h[:,0]))  (activation.py:8-12);  color_input [B_pad,32] f16 = [ half(SH_4(dirs)) | h[:,1:16] | 0 ]
 *   (network_ff.py:66-69), rows B..B_pad-1 zero (the FFMLP's row padding, ffmlp.py:156-158).  h [>=B,16] f16, dirs [B,3] f32.
 * backward: grad_h [B_pad,16] f16 from grad_sigma [B] f32 (activation.py:14-17) and grad_color_input [>=B,32] f16 (either may be NULL). */
NGP_API int ngp_ff_sigma_color_input(const uint16_t* h, const float* dirs, uint32_t B, uint32_t B_pad, float* sigma, uint16_t* color_input,
                             ngp_stream_t stream);
NGP_API int ngp_ff_sigma_color_input_backward(const uint16_t* h, const float* grad_sigma, const uint16_t* grad_color_input, uint32_t B,
                                      uint32_t B_pad, uint16_t* grad_h, ngp_stream_t stream);
/* rgb [B,3] f16 = sigmoid(outputs16[:, :3]) (network_ff.py:70,98: torch.sigmoid of the colour FFMLP's padded 16-wide output);
 * backward: grad_outputs16 [B_pad,16] f16, columns 3..15 and rows >= B zero. */
NGP_API int ngp_ff_rgb(const uint16_t* outputs16, uint32_t B, uint16_t* rgb, ngp_stream_t stream);
NGP_API int ngp_ff_rgb_backward(const uint16_t* grad_rgb, const uint16_t* rgb, uint32_t B, uint32_t B_pad, uint16_t* grad_outputs16,
                        ngp_stream_t stream);

/* ---------------- _ffmlp (ffmlp/src/ffmlp.h:8-15) ---------------- */

/* ffmlp.cu:636-709.  fp16 only.  inputs [B,input_dim], B % 16 == 0 (the wrapper pads to 128);
 * weights: flat blob [hidden x in | (num_layers-1) x hidden x hidden | output_dim x hidden];
 * forward_buffer [num_layers,B,hidden] (training) ; outputs [B,output_dim], output_dim == 16.
 * hidden_dim in {16,32,64,128,256}; input_dim % 16 == 0; activation codes as ffmlp/ffmlp.py:89-96. */
NGP_API int ngp_ffmlp_forward(const uint16_t* inputs, const uint16_t* weights, uint32_t B, uint32_t input_dim,
                      uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                      uint32_t output_activation, uint16_t* forward_buffer, uint16_t* outputs, ngp_stream_t stream);
/* (this build) ngp_ffmlp_forward / ngp_ffmlp_backward with the INPUT side in the hash-grid operator's level-major layout: inputs and
 * grad_inputs are [input_dim/2][B][2] (gridencoder.cu's [L,B,C], C == 2, B rows per plane) instead of [B,input_dim].  64-wide networks
 * (input_dim % 32 == 0, 2-4 layers); forward_buffer NULL = inference.  Everything else as the plain calls. */
NGP_API int ngp_ffmlp_forward_planes(const uint16_t* inputs, const uint16_t* weights, uint32_t B, uint32_t input_dim,
                             uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                             uint32_t output_activation, uint16_t* forward_buffer, uint16_t* outputs, ngp_stream_t stream);
NGP_API int ngp_ffmlp_backward_planes(const uint16_t* grad, const uint16_t* inputs, const uint16_t* weights, const uint16_t* forward_buffer,
                              uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                              uint32_t activation, uint32_t output_activation, int calc_grad_inputs, uint16_t* backward_buffer,
                              uint16_t* grad_inputs, uint16_t* grad_weights, void* workspace, size_t workspace_bytes,
                              ngp_stream_t stream);
/* (this build) 1 if ngp_ffmlp_backward(_planes) accepts forward_buffer == NULL for this shape: the hidden activations are then computed
 * again from `inputs` inside the backward kernel (the forward kernel's own instruction sequence: bit-identical values), so a training
 * forward can be an ngp_ffmlp_inference call that stores none.  64-wide networks, 2-4 layers, input_dim 32 or 64. */
NGP_API int ngp_ffmlp_backward_recomputes(uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers);
NGP_API int ngp_ffmlp_inference(const uint16_t* inputs, const uint16_t* weights, uint32_t B, uint32_t input_dim,
                        uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                        uint32_t output_activation, uint16_t* inference_buffer, uint16_t* outputs,
                        ngp_stream_t stream);
/* ffmlp.cu:745-897 ffmlp_backward (+ :410-520 kernel_mlp_fused_backward).  grad [B,16] fp16 is consumed as is (the
 * reference does not transfer the output activation either, ffmlp.cu:462-464).  backward_buffer [num_layers,B,hidden]:
 * slot j = dL/d(pre-activation) of forward_buffer[num_layers-1-j]; grad_weights (layout of `weights`) and, when
 * calc_grad_inputs, grad_inputs [B,input_dim] are overwritten.  Weight gradients are a deterministic split-K over the
 * batch: fp32 partials in the CALLER's `workspace` (device memory, 16-byte aligned, ngp_ffmlp_backward_workspace(...) bytes;
 * a smaller one -- at least one set of parameters, P * 4 bytes -- means fewer, longer batch chunks).  The library keeps no
 * state between calls: unlike the reference's static split-K streams (ffmlp.cu:721-741) concurrent backward calls on
 * different streams are independent.  Everything is enqueued on `stream`. */
NGP_API int ngp_ffmlp_backward(const uint16_t* grad, const uint16_t* inputs, const uint16_t* weights,
                       const uint16_t* forward_buffer, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                       uint32_t hidden_dim, uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                       int calc_grad_inputs, uint16_t* backward_buffer, uint16_t* grad_inputs,
                       uint16_t* grad_weights, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
NGP_API size_t ngp_ffmlp_backward_workspace(uint32_t B, uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers);
/* backward_buffer is scratch in the reference (ffmlp/ffmlp.py:70 allocates it, nothing reads it after the call).  The 64-wide
 * networks compute activation and weight gradients in one pass and never need it in memory: this returns the bytes a caller has
 * to provide -- 0 when backward_buffer may be NULL (a non-NULL buffer is still filled, as documented above). */
NGP_API size_t ngp_ffmlp_backward_buffer_bytes(uint32_t B, uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers);
/* ffmlp.cu:721-741: the reference creates CUTLASS split-K streams/events here.  Both are no-ops kept for the interface
 * (ffmlp/ffmlp.py:126 calls allocate_splitk from FFMLP.__init__): this library has no split-K state of its own. */
NGP_API int ngp_ffmlp_allocate_splitk(size_t n);
NGP_API int ngp_ffmlp_free_splitk(void);

/* ---------------- nerf/utils.py:52-116 get_rays (full frame, N <= 0 branch) ---------------- */

/* poses [Bc,4,4] f32 cam2world (device); rays_o/rays_d [Bc,H*W,3] f32.  Pixel centres +0.5,
 * dirs normalised then rotated, origin broadcast.  `pixel_inds` (int32 [n_pix] or NULL)
 * selects a pixel subset per camera (the Estimator's <=1024-pixel batches);
 * n_pix is H*W when pixel_inds is NULL. */
NGP_API int ngp_get_rays(const float* poses, uint32_t Bc, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                 const int32_t* pixel_inds, uint32_t n_pix, float* rays_o, float* rays_d, ngp_stream_t stream);
/* Vector-Jacobian product of the above with respect to the poses (what torch autograd gives for the reference's torch
 * ops, nerf/utils.py:103-111): grad_rays_o / grad_rays_d [Bc,n_pix,3] f32 (either may be NULL = zero) ->
 * grad_poses [Bc,4,4] f32, overwritten (row 3 is zero).  Deterministic. */
NGP_API int ngp_get_rays_backward(const float* grad_rays_o, const float* grad_rays_d, uint32_t Bc, float fx, float fy, float cx, float cy,
                          uint32_t H, uint32_t W, const int32_t* pixel_inds, uint32_t n_pix, float* grad_poses,
                          ngp_stream_t stream);

/* ---------------- fused render path behind NeRFRenderer.run_cuda (renderer.py:329-378) ---------------- */

/* Everything the eval-mode branch of run_cuda does between near_far_from_aabb and the
 * background mix, with the reference's exact per-iteration schedule
 * (n_step = clamp(N // n_alive, 1, 8), step += n_step while step < max_steps), executed
 * without a host round trip per iteration.
 *
 * Model description (device pointers, fp16 weights in the FFMLP blob layout):
 *   sigma net : 32 -> 64 x (1 + sigma_hidden_mm) -> 16   (ReLU, no output activation)
 *   colour net: 32 -> 64 x (1 + color_hidden_mm) -> 16   (first 3 outputs, sigmoid)
 *   colour input = [SH degree-4 (16) | geo_feat (15) | 0]  (nerf/network_ff.py:63-70);
 *   nerf/network.py's nn.Linear backbone is passed zero-padded to these shapes.
 */
typedef struct ngp_model {
    const uint16_t* embeddings;   /* [sO,2] fp16 hash table                               */
    const int32_t* offsets_host;  /* int32[L+1], host memory                              */
    uint32_t L;                   /* must be 16                                           */
    float S;                      /* log2(per_level_scale)                                */
    uint32_t H_base;              /* base resolution                                      */
    uint32_t gridtype;            /* 0 hash, 1 tiled                                      */
    int align_corners;
    const uint16_t* sigma_weights;/* blob: [64x32 | sigma_hidden_mm x 64x64 | 16x64]      */
    uint32_t sigma_hidden_mm;     /* 0..2                                                 */
    const uint16_t* color_weights;/* blob: [64x32 | color_hidden_mm x 64x64 | 16x64]      */
    uint32_t color_hidden_mm;     /* 0..3                                                 */
    float bound;                  /* scene bound; encoder input = (x+bound)/(2 bound)     */
    float density_scale;
    const uint8_t* density_bitfield; /* [C*H^3/8]                                         */
    uint32_t cascade;             /* C                                                    */
    uint32_t grid_size;           /* H (128): a power of two in [2, 1024]                 */
    const void* cell_tables;      /* optional (may be NULL): per-cell corner records of the first cell_levels levels, */
    uint32_t cell_levels;         /* built by ngp_build_cell_tables; the fused kernels use the records when this is 12 */
    const void* packed_weights;   /* the two blobs as MFMA fragments (ngp_pack_weights; ngp_packed_weights_bytes() bytes of device
                                     memory, 16-byte aligned), packed once per parameter version.  Required by
                                     ngp_network_forward / ngp_render_uniform; ngp_render_rays packs into its context when NULL */
    uint32_t precision;           /* NGP_PREC_F16 (0): fp16 table and weight blobs, as described above.  NGP_PREC_F32: `embeddings` is the
                                     fp32 table [sO,2] and the two blobs are fp32 in the same layout -- the arithmetic of the reference's
                                     rollout, which renders outside any autocast context (validate.py:288-291; gridencoder/grid.py:36-39
                                     and nn.Linear then stay fp32).  Served by ngp_pack_weights(_bwd), ngp_network_forward / _density
                                     (+ _backward) and ngp_render_uniform (+ _backward); the other fused entry points take fp16 */
} ngp_model;
#define NGP_PREC_F16 0u
#define NGP_PREC_F32 1u
/* fp16 as NGP_PREC_F16, but the fused gather interpolates with the reference's c10::Half arithmetic (every product w * entry rounded to
 * half, half running sum over the 8 corners, gridencoder.cu:169-172): the 32 features are then bit-identical to grid_encode's.  The
 * default accumulates the corners in fp32 and rounds once (closer to the exact value, one instruction per corner instead of three). */
#define NGP_PREC_F16_REF 2u

/* fragment-major copy of model->sigma_weights / color_weights for the fused kernels (layout: fused_net.hpp, k_pack_weights) */
NGP_API size_t ngp_packed_weights_bytes(void);
NGP_API int ngp_pack_weights(const ngp_model* model, void* out, ngp_stream_t stream);

/* Per-cell corner records: a derived copy of the first n_levels levels of the hash table in which every grid CELL owns the 8
 * entries its corners map to (32 contiguous bytes), so that the fused kernels read one record per sample and level instead of
 * gathering 8 entries from up to 4 cache lines.  The values are copies: results do not change.  It trades HBM capacity for
 * gather work (38 GB for 12 levels of the bound-2 Stonehenge table; the MI355X has 288 GB); rebuild it when the table changes.
 * ngp_cell_tables_bytes: size of the buffer for n_levels levels (0: not representable). */
NGP_API size_t ngp_cell_tables_bytes(const ngp_model* model, uint32_t n_levels);
NGP_API int ngp_build_cell_tables(const ngp_model* model, uint32_t n_levels, void* out, ngp_stream_t stream);

typedef struct ngp_render_stats {
    uint64_t samples_marched;     /* non-padding samples generated (sum over iterations)  */
    uint64_t samples_slots;       /* sum of n_alive*n_step, the reference's batch sizes   */
    uint32_t iterations;          /* python-loop iterations the reference would have run  */
    uint32_t rays;                /* N                                                    */
    uint32_t last_n_alive;        /* n_alive and n_step of the last iteration             */
    uint32_t last_n_step;
    uint32_t launches;            /* kernel launches enqueued (incl. run-ahead no-ops)    */
    uint32_t replayed;            /* launches that covered several reference iterations, failed their verification and were rolled back */
} ngp_render_stats;

typedef struct ngp_render_ctx ngp_render_ctx;  /* pinned status ring, events, scratch sizes */

/* creates the per-stream context for frames of at most max_rays rays (allocates device scratch
 * once: this is setup, not the data path) */
NGP_API int ngp_render_ctx_create(uint32_t max_rays, ngp_render_ctx** out);
NGP_API int ngp_render_ctx_destroy(ngp_render_ctx* ctx);

/* Scheduling hint: the rays of the following ngp_render_rays calls are the pixels of row-major frames `width` pixels wide
 * (what get_rays produces, nerf/utils.py:52-116); 0 = make no assumption (the default).  The renderer then starts its list of
 * live rays in 4x4-pixel tiles instead of row order, which makes the hash-grid gathers of neighbouring samples share cache
 * lines.  Results do not depend on it (the order of rays_alive enters no output when perturb == 0; with perturb the hint is
 * ignored, because march_rays seeds its jitter with the list index, raymarching.cu:819). */
NGP_API int ngp_render_ctx_set_frame_width(ngp_render_ctx* ctx, uint32_t width);

/* Diagnostics: switches of the launch sizing for this context's calls (0 = the default).  A context's own word,
 * apart from the debug flag word of enum ngp_debug_flag, whose set of bits is frozen.  Results do not depend on it; any other bit
 * is refused with NGP_EINVAL. */
#define NGP_SCHED_NO_FORECAST 1u    /* multi-iteration launches are sized by the recent death rate alone, not by the saturation forecast of the live rays */
NGP_API int ngp_render_ctx_set_schedule_flags(ngp_render_ctx* ctx, uint32_t flags);

/* Schedule counters of the context's most recent ngp_render_rays call -> out[0..7] (all zero before the first call).  Synchronises
 * the stream of that call, which must still exist.
 *   [0] launches that covered several reference iterations, failed their verification and were rolled back (ngp_render_stats::replayed)
 *   [1] network samples evaluated in those launches and discarded with them
 *   [2] reserved (0)
 *   [3] launches that the saturation forecast made smaller than the death rate alone would have (NGP_SCHED_NO_FORECAST: 0)
 *   [4] the last multi-iteration launch: deaths forecast before its last verified iteration, [5] deaths counted there
 *   [6] multi-iteration launches run (rolled-back ones included)
 *   [7] reserved (0) */
NGP_API int ngp_render_ctx_schedule_stats(ngp_render_ctx* ctx, uint64_t* out);

/* rays_o/rays_d [N,3] f32, nears/fars [N] f32 (from ngp_near_far_from_aabb).
 * Outputs weights_sum [N], depth [N], image [N,3] f32: the accumulated values BEFORE the
 * background mix / depth normalisation of renderer.py:375-378 (done by the caller as in the
 * reference).
 * last_sigmas [N+128] / last_rgbs [N+128,3] (both or neither; may be NULL): the `sigmas` (already
 * multiplied by density_scale) and `rgbs` tensors of the reference's LAST loop iteration
 * (renderer.py:383-384), slot-major n*n_step+k; padding slots hold pad_value[0] (sigma) and
 * pad_value[1..3] (rgb) -- what the network returns for the zero-filled padding rows.
 * stats_host may be NULL.  Synchronises `stream` before returning iff stats_host != NULL or sync != 0. */
NGP_API int ngp_render_rays(ngp_render_ctx* ctx, const ngp_model* model, const float* rays_o, const float* rays_d,
                    const float* nears, const float* fars, uint32_t N, float dt_gamma, uint32_t max_steps,
                    uint32_t perturb, float* weights_sum, float* depth, float* image, float* last_sigmas,
                    float* last_rgbs, const float* pad_value_host, ngp_render_stats* stats_host, int sync,
                    ngp_stream_t stream);

/* fused hash-grid encode + MLPs on an explicit point list: the body of NeRFNetwork.forward
 * (nerf/network_ff.py:51-75).  xyzs [M,3] in [-bound,bound], dirs [M,3]; sigmas [M] f32 (already
 * multiplied by nothing: raw trunc_exp output), rgbs [M,3] f32 (fp16-rounded sigmoid). M % 16 == 0 not required. */
NGP_API int ngp_network_forward(const ngp_model* model, const float* xyzs, const float* dirs, uint32_t M, float* sigmas,
                        float* rgbs, ngp_stream_t stream);

/* the density half alone (NeRFNetwork.density, nerf/network.py:126-143, nerf/network_ff.py:77-90): sigmas [M] f32, raw trunc_exp
 * output; geo_feat (may be NULL) [M,15] f32, the sigma net's outputs 1..15 the reference returns next to sigma */
NGP_API int ngp_network_density(const ngp_model* model, const float* xyzs, uint32_t M, float* sigmas, float* geo_feat, ngp_stream_t stream);
/* Its vector-Jacobian product with respect to the POINTS, map frozen: what the trajectory planner differentiates
 * (nav/quad_plot.py:223-249 through validate.py:288's density_fn: ~6 k body points, 250 Adam steps per simulator step).
 * grad_sigmas [M] and grad_geo_feat [M,15] (either may be NULL = zero) -> grad_xyzs [M,3] (overwritten).  One launch, nothing saved
 * by the forward call; packed_weights_bwd as for ngp_render_uniform_backward. */
NGP_API int ngp_network_density_backward(const ngp_model* model, const void* packed_weights_bwd, const float* xyzs, uint32_t M,
                                 const float* grad_sigmas, const float* grad_geo_feat, float* grad_xyzs, ngp_stream_t stream);

/* The trajectory planner's collision term (nav/quad_plot.py:216-241 with validate.py:288's density_fn) in one launch: for every
 * planned state s, its B body points go to the world (R_s b + p_s), to the NeRF's axes (@ rot), through the density half, and
 * out[s] = mean_b sigma^2.  rot_matrix [S,3,3], pos [S,3], body [B,3], rot [3,3] (row-major, device memory) -> out [S].
 * One workgroup per state with fixed-order sums: identical bits on every call.  No workspace. */
NGP_API int ngp_planner_collision(const ngp_model* model, const float* rot_matrix, const float* pos, const float* body, const float* rot,
                                  uint32_t S, uint32_t B, float* out, ngp_stream_t stream);
/* Its vector-Jacobian product, map frozen: grad_out [S] -> grad_pos [S,3], grad_rot_matrix [S,3,3] (overwritten).
 * packed_weights_bwd as for ngp_network_density_backward. */
NGP_API int ngp_planner_collision_backward(const ngp_model* model, const void* packed_weights_bwd, const float* rot_matrix, const float* pos,
                                           const float* body, const float* rot, uint32_t S, uint32_t B, const float* grad_out,
                                           float* grad_pos, float* grad_rot_matrix, ngp_stream_t stream);

/* The density behind the rollout's collision map (nerfsafetyvalidation_amd/collision.py; the reference marks mesh vertices in Blender
 * instead, validation/utils/createCollisionMap.py).  For cell (i, j, k) of an X x Y x Z box and sub-sample (a, b, c) in [0, s)^3 the
 * world point is p_x = start_x + ((float)i + ((float)a + 0.5f) / (float)s) / granularity (likewise y, z; fp32, IEEE division, no
 * contraction), mapped to the NeRF's axes as x[j] = p0 * rot[j] + p1 * rot[3 + j] + p2 * rot[6 + j] (rot [3,3] row-major).
 * out_max_sigma [X,Y,Z] (C order, device) = the largest raw sigma (trunc_exp output) over the s^3 points, each bit-identical to
 * ngp_network_density's on the same fp32 point; fp16 or fp32 network (ngp_model::precision).  start_host [3] and rot_host [9] are
 * host memory.  1 <= s <= 16, X * Y * Z < 2^31.  No workspace. */
NGP_API int ngp_cell_max_density(const ngp_model* model, const float* start_host, float granularity, uint32_t X, uint32_t Y, uint32_t Z,
                                 uint32_t s, const float* rot_host, float* out_max_sigma, ngp_stream_t stream);

/* Exact squared Euclidean distance transform of a C-order occupancy map: occupied uint8 [X,Y,Z] (non-zero = occupied) ->
 * d2 int32 [X,Y,Z] = the squared distance, in cells, from every cell to the nearest occupied cell (0 on occupied cells):
 * scipy.ndimage.distance_transform_edt(~map) ** 2 of validation/utils/createSDF.py, in integers.  A map with no occupied cell gives
 * NGP_EDT_INF in every cell (scipy measures from a phantom background outside the array there).  Three separable passes, integer
 * arithmetic only: the same bits on every call.  Every dimension in [1, 16384], X * Y * Z < 2^31.  workspace:
 * ngp_edt_sq_workspace(X, Y, Z) bytes, 4-byte aligned (NGP_EWORKSPACE when smaller). */
#define NGP_EDT_INF 0x7fffffff
NGP_API size_t ngp_edt_sq_workspace(uint32_t X, uint32_t Y, uint32_t Z);
NGP_API int ngp_edt_sq(const uint8_t* occupied, uint32_t X, uint32_t Y, uint32_t Z, int32_t* d2, void* workspace, size_t workspace_bytes,
                       ngp_stream_t stream);

/* Connected components of a C-order occupancy map (csrc/components.hip; the rule in full: nerfsafetyvalidation_amd/collision.py):
 * occupied uint8 [X,Y,Z], non-zero = occupied.  Two occupied cells are neighbours when their offset is one of `connectivity`'s:
 * 6, 18, 26 = the offsets of {-1,0,1}^3 \ 0 with at most 1, 2, 3 non-zero entries; 14 = +- the seven offsets of {0,1}^3 \ 0, the
 * lattice edges of the isosurface's Kuhn split.  scipy.ndimage.label's result for the matching structure, numbering included:
 *   ngp_label_components  labels int32 [X,Y,Z] = 0 on empty cells, else 1 + the rank of the cell's component, components ranked by the
 *                         smallest C-order linear index of their cells; *n_components (int32, DEVICE memory) = their number.  A
 *                         function of the input alone: the same bits on every call (integer min-atomics on a union-find forest whose
 *                         links always point to a smaller index; the outcome does not depend on their order).  Six launches and a
 *                         4-byte memset on `stream`, no host synchronisation.  Every device loop is bounded by the map's size; should
 *                         one reach its bound (a corrupted workspace), *n_components is -1, -2 or -3 (the stage: tile, seams,
 *                         flatten) and the labels are not valid -- ngp_component_stats refuses such an n with NGP_ELAUNCH and names
 *                         the stage in ngp_last_error.
 *   ngp_component_stats   for labels of n components (n: the value read back; n == 0 launches nothing): cells int64 [n] the number of
 *                         cells, lo / hi int32 [n,3] the inclusive index bounding box, overlap int64 [n] (with truth uint8 [X,Y,Z],
 *                         non-zero = marked; both may be null) the number of its cells that truth marks.  All device memory,
 *                         overwritten.  Equal labels are reduced within the wave before the integer atomics (add, min, max).
 * Every dimension >= 1, X * Y * Z < 2^31, connectivity one of the four: NGP_EINVAL otherwise, nothing launched.  workspace:
 * ngp_label_components_workspace(X, Y, Z) bytes (host arithmetic; 0 for a size it refuses), 4-byte aligned (NGP_EWORKSPACE when
 * smaller, nothing launched).  No global state: calls on different streams with their own workspaces do not interact.
 * NGP_COMPONENTS_TILE_*: the cells per axis of the tile one workgroup labels in LDS (tests place their seams by it). */
#define NGP_COMPONENTS_TILE_X 4
#define NGP_COMPONENTS_TILE_Y 4
#define NGP_COMPONENTS_TILE_Z 16
NGP_API size_t ngp_label_components_workspace(uint32_t X, uint32_t Y, uint32_t Z);
NGP_API int ngp_label_components(const uint8_t* occupied, uint32_t X, uint32_t Y, uint32_t Z, uint32_t connectivity, int32_t* labels,
                                 int32_t* n_components, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
NGP_API int ngp_component_stats(const int32_t* labels, uint32_t X, uint32_t Y, uint32_t Z, int32_t n, const uint8_t* truth, int64_t* cells,
                                int32_t* lo, int32_t* hi, int64_t* overlap, ngp_stream_t stream);

/* Isosurface of a C-order scalar lattice u float [X,Y,Z] as an indexed, welded triangle mesh: marching tetrahedra on the Kuhn split
 * (six tetrahedra around every cell's (0,0,0)-(1,1,1) diagonal; DESIGN.md "Mesh export" fixes the rule and the output order).  A
 * lattice point is inside iff u > threshold (NaN is outside); every lattice edge (3 axis edges, 3 face diagonals, 1 body diagonal per
 * point, owned by the lower end) whose ends differ carries one vertex at pa + (thr - ua) / (ub - ua) * (pb - pa), in index units.
 * Two calls with one host read between them:
 *   ngp_isosurface_count  fills the workspace (edge masks, triangle counts, their exclusive scans) and writes totals[0] = V and
 *                         totals[1] = F (device memory, two uint64);
 *   ngp_isosurface_emit   with the SAME u, sizes, threshold and workspace, and the V and F read back: vertices float [V,3] ordered by
 *                         (owner in C order, edge type), faces int32 [F,3] ordered by (cell in C order, tetrahedron, triangle),
 *                         normals from inside to outside.  V == F == 0 launches nothing (the outputs may be null).
 * Every axis >= 2, X * Y * Z < 2^31, V < 2^31 and F < 2^31 (NGP_EINVAL otherwise, nothing launched).  workspace:
 * ngp_isosurface_workspace(X, Y, Z) bytes (0 for sizes it refuses), 8-byte aligned (NGP_EWORKSPACE when smaller).  No atomics and
 * no global state: the same bits on every call, and calls on different streams with their own workspaces do not interact. */
NGP_API size_t ngp_isosurface_workspace(uint32_t X, uint32_t Y, uint32_t Z);
NGP_API int ngp_isosurface_count(const float* u, uint32_t X, uint32_t Y, uint32_t Z, float threshold, void* workspace, size_t workspace_bytes,
                                 uint64_t* totals, ngp_stream_t stream);
NGP_API int ngp_isosurface_emit(const float* u, uint32_t X, uint32_t Y, uint32_t Z, float threshold, const void* workspace,
                                size_t workspace_bytes, uint64_t V, uint64_t F, float* vertices, int32_t* faces, ngp_stream_t stream);

/* Mesh simplification by vertex clustering with quadric-optimal representatives (csrc/simplify.hip; DESIGN.md "Mesh simplification"
 * fixes the rule and the summation order; nerfsafetyvalidation_amd/mesh.py's _simplify_numpy defines the result, and these kernels
 * give its bits).  vertices float [V,3], faces int32 [F,3], cell > 0 and origin (three HOST doubles).  All arithmetic is IEEE double
 * on the float inputs, one rounding per operation.  A vertex belongs to cell i_a = floor((v_a - o_a) / cell), 0 <= i_a < 2^21, key =
 * ix << 42 | iy << 21 | iz; the clusters are the distinct keys, numbered in ascending order.  Sorting and scanning between the calls
 * are the caller's (stable sorts, so that every list is in ascending input index within a cluster); all arrays are device memory:
 *   ngp_simplify_keys        keys int64 [V].  A non-finite coordinate, a vertex below origin or an index >= 2^21 sets *error (int32,
 *                            zeroed by the caller; atomicMax) to 1 and the key to 0; a face index outside [0, V) sets it to 2.  The
 *                            later calls are memory-safe whatever the error; the caller reads the word once, with V' and F', and
 *                            reads nothing else when it is set.
 *   ngp_simplify_corners     vcluster int32 [V] (the cluster of every vertex) -> ccluster int32 [3 F], corner 3 f + k's cluster.
 *   ngp_simplify_accumulate  sorted_keys int64 [V] ascending; vertex_order int64 [V] the vertices sorted by cluster; vertex_start int64
 *                            [V + 1] the first row of cluster c in it (V for c >= the number of clusters); corner_order int64 [3 F],
 *                            corner_start int64 [V + 1] the same for the corners -> representatives float [V,3], row c for cluster c.
 *                            Relative to p_c = o + (i + 1/2) cell: m = the mean of the cluster's vertices; over its corners, with A, B,
 *                            C the corner's face: n = (B - A) x (C - A), d = -n . (A - p_c), Q_A += n n^T, q_b += d n.  Every sum: 64
 *                            consecutive ranks by the xor butterfly (offsets 32 .. 1, +0 beyond the list), the groups added in
 *                            ascending order to a double that starts at +0.  x solves (Q_A + mu I) x = mu m - q_b, mu =
 *                            NGP_SIMPLIFY_LAMBDA * trace(Q_A), by Cramer's rule; x = m for placement NGP_SIMPLIFY_MEAN, trace == 0, or
 *                            an x that is not finite or has some |x_a| > cell / 2; x is clamped to +- cell / 2 and the row is
 *                            float(p_c + x).  A cluster of one vertex keeps that vertex's bits.  One wave per cluster.
 *   ngp_simplify_faces       keep int32 [F] = 1 iff the face's three clusters differ, referenced int32 [V] = 1 for the clusters of kept
 *                            faces (zeroed here first).
 *   ngp_simplify_emit        with the inclusive scans of keep and referenced (int64) and their totals F' and V' read back: the kept
 *                            faces in input order and rotation, renumbered (duplicates stay); the referenced clusters' rows in
 *                            order; vertex_map int32 [V], the output vertex of every input vertex or -1.
 * V < 2^31, 3 F < 2^31, cell finite and > 0 (NGP_EINVAL otherwise, nothing launched).  No float atomics, no workspace, no global state:
 * the same bits on every call, and calls on different streams do not interact. */
#define NGP_SIMPLIFY_LAMBDA 1e-3
#define NGP_SIMPLIFY_QUADRIC 0
#define NGP_SIMPLIFY_MEAN 1
NGP_API int ngp_simplify_keys(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const double* origin3_host, double cell,
                              int64_t* keys, int32_t* error, ngp_stream_t stream);
NGP_API int ngp_simplify_corners(const int32_t* faces, uint32_t F, uint32_t V, const int32_t* vcluster, int32_t* ccluster, ngp_stream_t stream);
NGP_API int ngp_simplify_accumulate(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const double* origin3_host, double cell,
                                    int placement, const int64_t* sorted_keys, const int64_t* vertex_order, const int64_t* vertex_start,
                                    const int64_t* corner_order, const int64_t* corner_start, float* representatives, ngp_stream_t stream);
NGP_API int ngp_simplify_faces(const int32_t* ccluster, uint32_t F, uint32_t V, int32_t* keep, int32_t* referenced, ngp_stream_t stream);
NGP_API int ngp_simplify_emit(uint32_t V, uint32_t F, const int32_t* vcluster, const int32_t* ccluster, const float* representatives,
                              const int32_t* keep, const int64_t* keep_scan, const int32_t* referenced, const int64_t* referenced_scan,
                              uint64_t n_vertices, uint64_t n_faces, float* vertices_out, int32_t* faces_out, int32_t* vertex_map,
                              ngp_stream_t stream);

/* Rays against a triangle mesh through a uniform grid (DESIGN.md "The ground-truth world"; world.py).  tri_data float [F,12],
 * 16-byte aligned: per triangle the rows (v0, 0), (e1 = v1 - v0, 0), (e2 = v2 - v0, 0).  The grid is host arithmetic of the caller:
 * cell (a, b, c) covers lo + (a, b, c) * cell .. lo + (a + 1, b + 1, c + 1) * cell, 1..256 cells per axis, inv_cell = 1 / cell;
 * `grow` is added to every side of a triangle's bounding box before it is binned; a ray whose origin has a component beyond `reach`
 * in magnitude is tested against all F triangles instead of walking the grid.
 *   ngp_raycast_bin_count  counts int32 [F]: the number of cells triangle f's grown box overlaps.
 *   ngp_raycast_bin_emit   offsets int64 [F] = the exclusive scan of counts, P = their sum: pair_cell / pair_tri int32 [P], triangle
 *                          f's pairs at offsets[f].., its cells in C order.  The caller sorts the pairs by cell (stable: every
 *                          cell's triangles ascending) and builds cell_start int32 [nx ny nz + 1].
 *   ngp_raycast            rays_o / rays_d float [N,3] -> t float [N] (+inf on a miss), prim int32 [N] (-1 on a miss), u, v float [N]
 *                          (0 on a miss), by the hit rule of csrc/raycast.hip: Moeller-Trumbore, two-sided, one IEEE operation per
 *                          step, accepted iff u >= 0, v >= 0, u + v <= 1, t_min < t < t_max; the smallest t wins, equal t goes to the
 *                          lowest triangle index; a ray with a non-finite component or a zero direction misses.  The result does not
 *                          depend on the grid or on frame_width.  frame_width: 0, or the width W of the row-major frame(s) the rays
 *                          are (W divides N): a wave then takes an 8 x 8 pixel tile.  N == 0 launches nothing.
 *   ngp_raycast_shade      image float [N,3] and image_u8 uint8 [N,3] ((uint8)(x * 255)): the barycentric blend of the vertex colours
 *                          (colors float [V,3] with faces int32 [F,3]; both null: mid-grey) times ambient + (1 - ambient) |n . d| /
 *                          (|n| |d|), n = e1 x e2, clamped to [0, 1]; bg_color3_host (host memory) where prim < 0.
 * F, P, N < 2^31 (NGP_EINVAL otherwise, nothing launched).  No atomics, no workspace, no global state. */
typedef struct ngp_raycast_grid {
    float lo[3], cell[3], inv_cell[3], grow[3];
    float reach;
    uint32_t n[3];
} ngp_raycast_grid;
NGP_API int ngp_raycast_bin_count(const float* tri_data, uint32_t F, const ngp_raycast_grid* grid, int32_t* counts, ngp_stream_t stream);
NGP_API int ngp_raycast_bin_emit(const float* tri_data, uint32_t F, const ngp_raycast_grid* grid, const int64_t* offsets, uint64_t P,
                                 int32_t* pair_cell, int32_t* pair_tri, ngp_stream_t stream);
NGP_API int ngp_raycast(const float* rays_o, const float* rays_d, uint64_t N, const ngp_raycast_grid* grid, const int32_t* cell_start,
                        const int32_t* pair_tri, uint64_t P, const float* tri_data, uint32_t F, float t_min, float t_max,
                        uint32_t frame_width, float* t, int32_t* prim, float* u, float* v, ngp_stream_t stream);
NGP_API int ngp_raycast_shade(const float* rays_d, const int32_t* prim, const float* u, const float* v, uint64_t N, const float* tri_data,
                              const int32_t* faces, uint32_t F, const float* colors, uint32_t V, float ambient,
                              const float* bg_color3_host, float* image, uint8_t* image_u8, ngp_stream_t stream);

/* The mesh as a collision map (nerfsafetyvalidation_amd/world.py, MeshWorld.occupancy): map uint8 [X,Y,Z] (C order, device) = 1 in
 * every cell of the box that a triangle touches, 0 elsewhere -- a conservative surface voxelisation, the input of ngp_edt_sq.
 * vertices float [V,3] (the mesh's axes), faces int32 [F,3].  The box: cell (i, j, k) has the centre start + ((i, j, k) + 0.5) /
 * granularity and the half-width 0.5 / granularity, in the world frame; world axis a of a vertex is sign[a] * vertex[axis[a]] (axis
 * a permutation of 0, 1, 2, sign +1 or -1: exact).  From there on float64, one IEEE operation per step (the rule: csrc/voxelize.hip):
 * a cell is marked iff the closed triangle-box separating-axis test (13 axes, strict inequalities: touching is overlap) finds no
 * separating axis for some face, or it holds one of a face's vertices (floor((w - start) * granularity)).  A face with an index
 * outside the V vertices marks nothing.
 *   ngp_voxelize_count  zeroes the map (on the stream), marks the vertices' cells and writes counts int32 [F]: the number of
 *                       candidate cells of face f (its bounding box in cells, one cell wider on every side, clipped to the box).
 *   ngp_voxelize_mark   ends int64 [F] = the inclusive scan of counts: one lane per (face, candidate cell) pair for the pairs
 *                       pair_base .. pair_base + n_pairs - 1 of that order (n_pairs < 2^31 per call; a caller with more pairs calls
 *                       again with the next pair_base), with the SAME vertices, faces and box.  n_pairs == 0 launches nothing.
 * The result does not depend on how the pairs are split into calls.  X * Y * Z < 2^31, V, F < 2^31 (NGP_EINVAL otherwise, nothing
 * launched).  No atomics (the only writes to the map are byte stores of the constant 1), no workspace, no global state. */
typedef struct ngp_voxel_box {
    double start[3];
    double granularity;
    uint32_t shape[3];
    int32_t axis[3], sign[3];
} ngp_voxel_box;
NGP_API int ngp_voxelize_count(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const ngp_voxel_box* box, uint8_t* map,
                               int32_t* counts, ngp_stream_t stream);
NGP_API int ngp_voxelize_mark(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const ngp_voxel_box* box,
                              const int64_t* ends, uint64_t pair_base, uint64_t n_pairs, uint8_t* map, ngp_stream_t stream);

/* The drone's body as an oriented box (csrc/body.hip; MeshWorld.box_overlap, collision.box_cells).  boxes double [N,15], device,
 * 8-byte aligned: per row the centre c (3), R row-major (9: its columns are the box's axes in the world frame) and the half extents h
 * (3).  float64, one IEEE operation per step, by "The body rule" of nerfsafetyvalidation_amd/world.py's docstring; a row with a
 * non-finite entry or a negative half extent overlaps nothing.  No rotation is computed here.
 *   ngp_box_mesh_overlap   prim int32 [N]: the lowest index of a triangle the box overlaps (closed 13-axis box-triangle test in the
 *                          box's frame, touching is overlap), or -1.  tri_verts float [F,12], 16-byte aligned, the exact vertices
 *                          (ngp_closest_point's table), in the mesh's axes; world axis a of a vertex is sign3_host[a] *
 *                          vertex[axis3_host[a]] (three ints each, HOST memory, ngp_voxel_box's axis / sign).  grid, cell_start,
 *                          pair_tri, P: the grid ngp_raycast walks; it only chooses candidates, no result depends on it.
 *   ngp_box_cells_overlap  cell int32 [N]: the lowest C-order linear index of a non-zero cell of map uint8 [X,Y,Z] that the box
 *                          overlaps (closed 15-axis box-box test, touching is overlap), or -1.  box: the map's start, granularity
 *                          and shape (axis and sign are not read); cells outside the map do not exist.
 * N == 0 launches nothing.  N, F, P, X * Y * Z < 2^31 (NGP_EINVAL otherwise, nothing launched).  One wave per box; no atomics, no
 * workspace, no global state. */
NGP_API int ngp_box_mesh_overlap(const double* boxes, uint64_t N, const ngp_raycast_grid* grid, const int32_t* cell_start,
                                 const int32_t* pair_tri, uint64_t P, const float* tri_verts, uint32_t F, const int32_t* axis3_host,
                                 const int32_t* sign3_host, int32_t* prim, ngp_stream_t stream);
NGP_API int ngp_box_cells_overlap(const uint8_t* map, const ngp_voxel_box* box, const double* boxes, uint64_t N, int32_t* cell,
                                  ngp_stream_t stream);

/* The gap between the body box and the nearest obstacle (csrc/clearance.hip; MeshWorld.box_clearance, collision.box_cells_clearance),
 * by "The clearance rule" of nerfsafetyvalidation_amd/world.py's docstring: float64, one IEEE operation per step.  The arguments of
 * the two entry points above, and:
 *   max_distance  a length > 0 or +inf: a distance above it is not accepted.  It also bounds the candidates; no result depends on them.
 *   distance      double [N], device, 8-byte aligned: the distance from the box to the nearest triangle (occupied cell), 0 where they
 *                 overlap, +inf where nothing lies within max_distance or the row is invalid.
 *   prim / cell   int32 [N]: the lowest index among the nearest, -1 with distance +inf; it is `hit` wherever hit >= 0.
 *   hit           int32 [N]: what ngp_box_mesh_overlap's prim (ngp_box_cells_overlap's cell) is for the same box -- the same test.
 * N == 0 launches nothing.  NGP_EINVAL, with a message and nothing launched, when N >= 2^31, when max_distance is NaN or <= 0, or when
 * a pointer is null with N > 0.  One wave per box; no atomics, no workspace, no global state. */
NGP_API int ngp_box_mesh_clearance(const double* boxes, uint64_t N, const ngp_raycast_grid* grid, const int32_t* cell_start,
                                   const int32_t* pair_tri, uint64_t P, const float* tri_verts, uint32_t F, const int32_t* axis3_host,
                                   const int32_t* sign3_host, double max_distance, double* distance, int32_t* prim, int32_t* hit,
                                   ngp_stream_t stream);
NGP_API int ngp_box_cells_clearance(const uint8_t* map, const ngp_voxel_box* box, const double* boxes, uint64_t N, double max_distance,
                                    double* distance, int32_t* cell, int32_t* hit, ngp_stream_t stream);

/* Rays against a list of analytic primitives, merged by depth with a mesh cast (csrc/overlay.hip): the replay's failure view.
 * The table: 8 floats per primitive, kind, a.xyz, b.xyz, r -- kind 0 a capsule with the axis a-b and the radius r, kind 1 an
 * axis-aligned box with the centre a and the half extents b.  prims_host is the table in HOST memory, validated before anything is
 * launched (any other kind, a non-finite field or r <= 0: NGP_EINVAL); prims is the same table in device memory, 16-byte aligned.
 *   ngp_overlay_cast   rays_o / rays_d float [N,3], t_max float [N] or null (+inf): the far limit per ray, the mesh cast's t of the
 *                      same ray -> t float [N] (+inf on a miss), prim int32 [N] (-1), normal float [N,3] (unnormalised; 0 on a
 *                      miss), by the hit rule of csrc/overlay.hip: the ray re-centred on the primitive, nearer roots only, accepted
 *                      iff t_min < t < t_max[ray]; the smallest t wins, equal t goes to the lowest index; a ray with a non-finite
 *                      component or a zero direction misses.  frame_width as ngp_raycast's.  P == 0 writes misses; N == 0
 *                      launches nothing.  The result does not depend on frame_width or on how the table is staged.
 *   ngp_overlay_shade  where 0 <= prim < P: image float [N,3] and image_u8 uint8 [N,3] ((uint8)(x * 255)) are overwritten with
 *                      colors float [P,3] of the primitive times ambient + (1 - ambient) |n . d| / (|n| |d|), clamped to [0, 1];
 *                      every other pixel keeps its bits.
 * N, P < 2^31 (NGP_EINVAL otherwise, nothing launched).  No atomics, no workspace, no global state. */
NGP_API int ngp_overlay_cast(const float* rays_o, const float* rays_d, uint64_t N, const float* prims_host, const float* prims, uint32_t P,
                             float t_min, const float* t_max, uint32_t frame_width, float* t, int32_t* prim, float* normal,
                             ngp_stream_t stream);
NGP_API int ngp_overlay_shade(const float* rays_d, const int32_t* prim, const float* normal, uint64_t N, const float* colors, uint32_t P,
                              float ambient, float* image, uint8_t* image_u8, ngp_stream_t stream);

/* The closest point of the mesh to every query point (csrc/closest.hip; MeshWorld.closest), on the grid ngp_raycast walks.
 * tri_verts float [F,12], 16-byte aligned: the rows (v0, 0), (v1, 0), (v2, 0) of the EXACT vertices (not tri_data: v0 + e1 is not v1).
 *   ngp_closest_point  points float [N,3] -> distance float [N], prim int32 [N], point float [N,3] by the closest-point rule of
 *                      nerfsafetyvalidation_amd/world.py's docstring: per triangle the smallest of an interior candidate and three
 *                      segment candidates, float32, one IEEE operation per step; the smallest finite d^2 wins, equal d^2 goes to the
 *                      lowest triangle index; accepted iff sqrt(d^2) <= max_distance (+inf allowed, NaN refused).  A point with a
 *                      non-finite component or without an accepted triangle is a miss: distance +inf, prim -1, point NaN.  A point
 *                      with a component beyond grid.reach is tested against all F triangles.  tested uint32 [N] or null: the number
 *                      of (point, triangle) pairs evaluated, a measurement.  No result depends on the grid.  N == 0 launches nothing.
 * F, P, N < 2^31 (NGP_EINVAL otherwise, nothing launched).  No atomics, no workspace, no global state.
 *
 *   ngp_distance_stats the running statistics of a sequence of distances handed over in any number of calls: this call appends
 *                      distance float [n] (device) to the `seen` elements of the earlier calls (seen == 0: a fresh sequence; the
 *                      state need not be cleared).  state: ngp_distance_stats_state_bytes() bytes of device memory, the caller's,
 *                      one per sequence.  thresholds_host: K <= NGP_DISTANCE_STATS_MAX_THRESHOLDS floats in host memory, the same
 *                      in every call of a sequence.  stats double [16] (device), of ALL seen + n elements:
 *                        [0] the number of finite entries  [1] their sum  [2] their sum of squares  [3] their maximum (0 without any)
 *                        [4 + k] the number of finite entries <= thresholds[k]  (0 for k >= K)  [12] seen + n  [13..15] 0
 *                      Fixed order, a function of an element's index in the sequence alone: the 64 elements of a group by the xor
 *                      butterfly in double; lane l of one wave adds the groups l, l + 64, ... in that order; the butterfly over the
 *                      64 lanes.  The same bits for any split of the sequence into calls.  Workspace:
 *                      ngp_distance_stats_workspace(n) bytes, 8-byte aligned (NGP_EWORKSPACE when smaller).  n < 2^31 per call.
 *                      No atomics.  Calls of one sequence go to one stream, in order. */
#define NGP_DISTANCE_STATS_MAX_THRESHOLDS 8
NGP_API int ngp_closest_point(const float* points, uint64_t N, const ngp_raycast_grid* grid, const int32_t* cell_start,
                              const int32_t* pair_tri, uint64_t P, const float* tri_verts, uint32_t F, float max_distance, float* distance,
                              int32_t* prim, float* point, uint32_t* tested, ngp_stream_t stream);
NGP_API size_t ngp_distance_stats_state_bytes(void);
NGP_API size_t ngp_distance_stats_workspace(uint64_t n);
NGP_API int ngp_distance_stats(const float* distance, uint64_t n, uint64_t seen, const float* thresholds_host, uint32_t K, void* state,
                               double* stats, void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* NeRFRenderer.run (nerf/renderer.py:125-258) for upsample_steps == 0 and perturb == False (fp16 or fp32 network, ngp_model::precision): T uniform
 * samples per ray between nears and fars (lin = the T values of torch.linspace(0, 1, T), device memory), hash grid + sigma net
 * on every sample, transmittance scan, colour net where weight > 1e-4, and the per-ray sums.  Outputs: weights_sum [N],
 * depth [N] (sum of weights * clamp((z - near) / (far - near), 0, 1)), image [N,3] (BEFORE the background mix),
 * aggregated_density [N]; for rays >= dump_begin also the per-sample sigmas [(N - dump_begin) * T] and
 * rgbs [(N - dump_begin) * T, 3] (the reference returns those of the last ray chunk only); both may be NULL. */
NGP_API int ngp_render_uniform(const ngp_model* model, const float* rays_o, const float* rays_d, const float* nears,
                       const float* fars, uint32_t N, uint32_t T, const float* lin, float* weights_sum, float* depth,
                       float* image, float* aggregated_density, uint32_t dump_begin, float* sigmas, float* rgbs,
                       uint32_t frame_width, ngp_stream_t stream);
/* frame_width: optional scheduling hint (0 = none) as in ngp_render_ctx_set_frame_width -- the rays are the pixels of row-major
 * frames this wide, so the kernel can take its groups of sixteen rays as 4x4-pixel blocks.  Results do not depend on it. */

/* The same with the NeRF-style importance resampling of nerf/renderer.py:172-204 in evaluation mode (sample_pdf :12-46 with det=True):
 * T uniform samples, U more drawn from the piecewise-constant PDF of the coarse weights (u = the U values of
 * torch.linspace(0.5 / U, 1 - 0.5 / U, U), device memory), both runs merged in depth order and composited together.  Outputs as
 * ngp_render_uniform, with T + U samples per ray in the optional sigmas / rgbs.  T >= 3; (5 T + 4 U) floats of LDS per ray must fit
 * beside the weights (T = U = 1024 does; the call refuses what does not). */
NGP_API int ngp_render_upsample(const ngp_model* model, const float* rays_o, const float* rays_d, const float* nears,
                        const float* fars, uint32_t N, uint32_t T, uint32_t U, const float* lin, const float* u,
                        float* weights_sum, float* depth, float* image, float* aggregated_density, uint32_t dump_begin,
                        float* sigmas, float* rgbs, uint32_t frame_width, void* workspace, size_t workspace_bytes,
                        ngp_stream_t stream);
/* frame_width: the scheduling hint of ngp_render_uniform.  workspace (optional, caller-owned device memory of
 * ngp_render_upsample_workspace(N, T, U) bytes; 0 = this batch size does not use one): with it, large batches run as four
 * launches -- both density passes and the merge + compositing with tiles across neighbouring rays, the resampling per ray in
 * between -- instead of one launch per ray.  Same samples (bit-identical sigmas / rgbs), per-ray sums to fp32 summation order. */
NGP_API size_t ngp_render_upsample_workspace(uint32_t N, uint32_t T, uint32_t U);

/* Vector-Jacobian product of ngp_render_uniform with respect to the RAYS with the map (table, weights) frozen: what
 * nav/estimator_helpers.py:191-225 differentiates (pose gradients through get_rays -> render -> run, <= 1024 pixels x 512 samples).
 * One launch, nothing saved by the forward call: grad_image [N,3] (of the image BEFORE the background mix), grad_depth /
 * grad_weights_sum / grad_aggregated_density [N] (each may be NULL = zero) -> grad_rays_o, grad_rays_d [N,3] (overwritten).
 * packed_weights_bwd: ngp_pack_weights_bwd(model, buf) -- the transposed weights as MFMA fragments
 * (ngp_packed_weights_bwd_bytes() bytes, 16-byte aligned), packed once per parameter version.  T <= 1024 and the LDS budget
 * (160 KB: both weight sets + 12 B per sample and resident wave) must hold, else NGP_EINVAL: T <= 512 for the reference's networks. */
NGP_API size_t ngp_packed_weights_bwd_bytes(void);
NGP_API int ngp_pack_weights_bwd(const ngp_model* model, void* out, ngp_stream_t stream);
/* bytes of LDS ngp_render_uniform_backward needs for this model and T samples per ray ((size_t)-1: a shape it does not serve);
 * the call fits when this is <= 160 KB */
NGP_API size_t ngp_render_uniform_backward_lds(const ngp_model* model, uint32_t T);
NGP_API int ngp_render_uniform_backward(const ngp_model* model, const void* packed_weights_bwd, const float* rays_o, const float* rays_d,
                                const float* nears, const float* fars, uint32_t N, uint32_t T, const float* lin, const float* grad_image,
                                const float* grad_depth, const float* grad_weights_sum, const float* grad_aggregated_density,
                                float* grad_rays_o, float* grad_rays_d, ngp_stream_t stream);

/* ---------------- sample bookkeeping of NeRFRenderer.run (nerf/renderer.py:12-46, 125-258), operator form ---------------- */

/* :148-160.  z_vals [N,T] = nears + (fars - nears) * lin[t] (lin = the T values of torch.linspace(0, 1, T), device memory), plus
 * (noise[n,t] - 0.5) * (fars - nears) / steps_for_dist when noise != NULL (:153-155; steps_for_dist = num_steps, 0 = T);
 * xyzs [N,T,3] = min(max(rays_o + rays_d * z, aabb[:3]), aabb[3:]).  With z_in != NULL the positions are given ([N,T], e.g. the
 * upsampled samples of :181-182) and only xyzs is produced.  aabb_host: 6 floats in host memory. */
NGP_API int ngp_uniform_samples(const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N, uint32_t T,
                        uint32_t steps_for_dist, const float* lin, const float* noise, const float* z_in, const float* aabb_host,
                        float* z_vals, float* xyzs, ngp_stream_t stream);
/* vector-Jacobian product of the above w.r.t. the rays (what autograd gives for :159-160, ties of the clip split as torch does):
 * grad_xyzs [N,T,3] -> grad_rays_o, grad_rays_d [N,3] (overwritten).  z_vals carry no gradient (nears / fars are computed under no_grad, :141). */
NGP_API int ngp_uniform_samples_backward(const float* grad_xyzs, const float* rays_o, const float* rays_d, const float* z_vals, uint32_t N,
                                 uint32_t T, const float* aabb_host, float* grad_rays_o, float* grad_rays_d, ngp_stream_t stream);
/* :206-210.  deltas = z[t+1] - z[t] (last: sample_dist[n]); alpha = 1 - exp(-delta * density_scale * sigma);
 * weights [N,T] = alpha * cumprod(1 - alpha + 1e-15) (exclusive). */
NGP_API int ngp_transmittance_weights(const float* z_vals, const float* sigmas, const float* sample_dist, uint32_t N, uint32_t T,
                              float density_scale, float* weights, ngp_stream_t stream);
/* grad_weights [N,T] -> grad_sigmas [N,T] (overwritten); T <= 4096 */
NGP_API int ngp_transmittance_weights_backward(const float* grad_weights, const float* z_vals, const float* sigmas, const float* sample_dist,
                                       uint32_t N, uint32_t T, float density_scale, float* grad_sigmas, ngp_stream_t stream);
/* sample_pdf (:12-46): bins [N,n_bins], weights [N,n_bins-1], u [n_samples] (u_per_ray == 0, the `det` linspace) or [N,n_samples]
 * -> samples [N,n_samples].  2 <= n_bins <= 4096. */
NGP_API int ngp_sample_pdf(const float* bins, const float* weights, uint32_t N, uint32_t n_bins, const float* u, int u_per_ray,
                   uint32_t n_samples, float* samples, ngp_stream_t stream);
/* the re-ordering of :190-198 for two runs that are each ascending along the ray: z [N,Ta+Tb] ascending, index [N,Ta+Tb] int64 =
 * position of every output in cat([z_a, z_b], 1) (ties: z_a first).  Equals torch.sort of the concatenation. */
NGP_API int ngp_merge_sorted(const float* z_a, const float* z_b, uint32_t N, uint32_t Ta, uint32_t Tb, float* z, int64_t* index,
                     ngp_stream_t stream);

/* ---------------- density-grid maintenance (nerf/renderer.py:388-544): the producer of density_bitfield ---------------- */

/* mark_untrained_grid (:388-449): cells of density_grid [cascade, H^3] (Morton order) whose centre no camera sees become -1.
 * poses [n_cams,4,4] cam2world (device).  workspace: ngp_mark_untrained_grid_workspace(n_cams, cascade, H) bytes, 4-byte aligned:
 * 0 up to 2048 cameras (one launch; NULL is fine), a flag word per cell (cascade * H^3 * 4 bytes) carried between the launches above
 * that, and 0 for a grid the call refuses.  NGP_EWORKSPACE when smaller.
 * H: a power of two in [2, 1024], cascade in [1, 8] (see ngp_march_rays_train), here and in ngp_density_grid_update / _finish. */
NGP_API size_t ngp_mark_untrained_grid_workspace(uint32_t n_cams, uint32_t cascade, uint32_t H);
NGP_API int ngp_mark_untrained_grid(const float* poses, uint32_t n_cams, float fx, float fy, float cx, float cy, float bound, uint32_t cascade,
                            uint32_t H, float* density_grid, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
/* sample positions of update_extra_state (:479-485, :512-520): coords int32 [n,3] cell coordinates, or NULL = every cell in the
 * reference's meshgrid order (x slowest); cascade_bound = min(2^cas, bound); noise [n,3] uniform [0,1) or NULL (cell centres)
 * -> xyzs [n,3] = centre * (cascade_bound - hgs) + (noise * 2 - 1) * hgs, indices int32 [n] = morton3D(coords). */
NGP_API int ngp_density_grid_points(const int32_t* coords, uint32_t n, uint32_t H, float cascade_bound, const float* noise, float* xyzs,
                            int32_t* indices, ngp_stream_t stream);
/* :489-491 + :531-532 for one cascade: tmp[indices] = sigmas * density_scale (duplicates: the LAST sample wins, as PyTorch's CPU
 * index_put_), then grid = max(grid * decay, tmp) where both are >= 0.  workspace: ngp_density_grid_workspace(cascade, H) bytes, 8-byte
 * aligned, shared with ngp_density_grid_finish: H^3 scatter words, then cascade * ceil(H^3 / 256) partial sums (NGP_EWORKSPACE when
 * smaller, from either call). */
NGP_API size_t ngp_density_grid_workspace(uint32_t cascade, uint32_t H);
NGP_API int ngp_density_grid_update(float* density_grid, uint32_t cascade, uint32_t H, uint32_t cas, const int32_t* indices, const float* sigmas,
                            uint32_t n, float density_scale, float decay, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
/* :533-538: mean_thresh[0] = mean(clamp(density_grid, 0)) (summed in double in a fixed order), mean_thresh[1] = min(mean,
 * density_thresh), bitfield = packbits(density_grid, mean_thresh[1]) -- on the device, no host round trip in between. */
NGP_API int ngp_density_grid_finish(const float* density_grid, uint32_t cascade, uint32_t H, float density_thresh, float* mean_thresh,
                            uint8_t* bitfield, void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* ---------------- uncertainty/quantification/gaussian_approximation_density_uncertainty.py:24-51 ---------------- */

/* Sufficient statistics of the Gaussian-approximation objective, one pass on the device instead of five global
 * reductions + .item() per scipy.minimize evaluation.  c [n,3] per-sample colours (dtype code 0 = f32,
 * 1 = f16), d [n] f32 per-sample densities, r [m] f32 rendered colour values.  stats (device, 8 doubles):
 *   [0] sum c^2 d^2   [1] sum c d   [2] sum r   [3] m   [4] sum d   [5] sum d^2   [6] n   [7] 0
 * accumulated in double in a fixed order (deterministic).  workspace: ngp_uq_stats_workspace() bytes of device memory, 8-byte aligned
 * (NGP_EWORKSPACE when smaller). */
NGP_API size_t ngp_uq_stats_workspace(void);
NGP_API int ngp_uq_stats(const void* c, int c_dtype, const float* d, uint64_t n, const float* r, uint64_t m, double* stats,
                 void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* ---------------- uncertainty/quantification/bayesian_laplace.py:38-91 (the Bayesian-Laplace fit's objective) ---------------- */

/* Negative log posterior of the fp32 linear sigma net (32 -> 64 -> 16, no bias) on CACHED encoder features:
 *   L(theta) = 0.5 sum_j (theta_j - prior_mean)^2 / prior_var + 0.5 sum_i (y_i - exp(h_i0))^2,   h_i = W2 relu(W1 f_i)
 * features float [n,32] (16-byte aligned; the grid encoder's output, zero rows for points outside the box), y float [n],
 * theta float [3072] = [W1 64x32 | W2 16x64] in nn.Linear order.  mode 0: *loss (double) only; 1: + grad float [3072] = the prior term
 * alone, exactly (theta - prior_mean) / (float)prior_var (what the reference's detached likelihood leaves of the gradient);
 * 2: + the likelihood's gradient, with trunc_exp's backward d sigma / d h = exp(clamp(h, -15, 15)) (rows 1..15 of W2: prior only).
 * Persistent workgroups over 64-point tiles, at most max_workgroups of them (0 = default, <= 4096), one partial each in `workspace`
 * (ngp_sigma_fit_workspace(n, max_workgroups) bytes, 8-byte aligned; NGP_EWORKSPACE when smaller), summed in a fixed order with the
 * loss in double: no atomics, the same bits on every call with the same arguments. */
NGP_API size_t ngp_sigma_fit_workspace(uint32_t n, uint32_t max_workgroups);
NGP_API int ngp_sigma_fit_eval(const float* features, const float* y, uint32_t n, const float* theta, float prior_mean, double prior_var,
                       int mode, uint32_t max_workgroups, void* workspace, size_t workspace_bytes, double* loss, float* grad,
                       ngp_stream_t stream);
/* One step of the fit without a host read-back (mode 1 or 2): the evaluation above at theta, history[history_index] = (float)loss,
 * `if loss < *min_loss: *min_loss = loss, *improved = 1` on that float (before the update, bayesian_laplace.py:75-81), then
 * ngp_adam_step on theta with torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8), learning rate lr and step count `step` >= 1.
 * grad, exp_avg, exp_avg_sq: float [3072] device buffers the caller keeps between steps (the moments zeroed before step 1). */
NGP_API int ngp_sigma_fit_step(const float* features, const float* y, uint32_t n, float* theta, float prior_mean, double prior_var, int mode,
                       uint32_t max_workgroups, void* workspace, size_t workspace_bytes, float* grad, float* exp_avg, float* exp_avg_sq,
                       float lr, uint32_t step, float* min_loss, int32_t* improved, float* history, uint32_t history_index,
                       ngp_stream_t stream);

/* ---------------- optimiser step of Trainer.train_step (nerf/utils.py:404-487; main_nerf.py:116) ---------------- */

/* torch.optim.Adam(betas, eps) without weight decay / amsgrad on one fp32 tensor, in place: exp_avg and exp_avg_sq are the
 * optimiser state, `step` counts from 1 (bias corrections 1 - beta^step), the gradient is divided by grad_scale first
 * (GradScaler.unscale_; pass 1).  One streaming pass, 28 B per parameter. */
NGP_API int ngp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, float lr, float beta1,
                  float beta2, float eps, uint32_t step, float grad_scale, ngp_stream_t stream);

/* The same step with its scalars on the device: `step_dev` (a float holding the step count: ngp_adam_advance_step adds 1 to it unless
 * *found_inf_dev != 0 -- call it once per optimiser step, before the tensors' updates), `grad_scale_dev` (the loss scale the gradients carry,
 * NULL = 1) and `found_inf_dev` (non-zero: skip the update; NULL = never) are what torch.amp.GradScaler hands to an optimiser that declares
 * _step_supports_amp_scaling.  No value of the step is read by the host: the training loop is not synchronised by its optimiser. */
NGP_API int ngp_adam_advance_step(float* step_dev, const float* found_inf_dev, ngp_stream_t stream);
NGP_API int ngp_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, float lr, float beta1,
                      float beta2, float eps, const float* step_dev, const float* grad_scale_dev, const float* found_inf_dev,
                      ngp_stream_t stream);

/* ---------------- data side of Trainer.train_step / eval_step (nerf/utils.py:426-480, nerf/provider.py:311-316) ---------------- */

/* Ground-truth colours of one batch of rays out of the resident image store, one thread per ray:
 *   gt_rgb[i] = rgb * a + bg * (1 - a)   (C == 4; utils.py:442)      gt_rgb[i] = rgb   (C == 3)
 * store: [n_img][n_pix][C] of store_dtype 0 = f32, 1 = f16, 2 = uint8 (a code k stands for (float)k / 255, the provider's
 * `image.astype(np.float32) / 255`); C in {3, 4}.  frame_base: index of the frame's first PIXEL in the store (frame * n_pix); inds
 * int64 [N] pixel ids inside the frame, or NULL = pixels 0 .. N-1 in order (evaluation: N = n_pix).  An id outside [0, n_pix) reads
 * nothing and gives NaN.  bg float [N,3], or NULL = white.  table: NULL, or 256 floats that replace k / 255 for the COLOUR channels
 * of a uint8 store (the linear colour space: srgb_to_linear of the 256 codes, utils.py:430-431; alpha is never converted) -- refused
 * for the other store types.  round_half != 0, or an f16 store: the reference holds the images in half (provider.py:250-254) and the
 * blend above is half arithmetic, every operation rounded to half; otherwise every operation is one fp32 operation (no fused
 * multiply-add).  gt_rgb float [N,3]. */
NGP_API int ngp_train_targets(const void* store, int store_dtype, uint32_t C, uint64_t frame_base, uint32_t n_pix, const int64_t* inds,
                      uint32_t N, const float* bg, const float* table, int round_half, float* gt_rgb, ngp_stream_t stream);

/* The depth targets of one batch of rays out of the resident 16-bit depth store (nerf/targets.py DepthStore), one thread per ray:
 * store uint16 [n_img][n_pix] codes of z-depth along the optical axis; frame_base: index of the frame's first pixel in the store;
 * inds int64 [N] pixel ids inside the frame (duplicates allowed), or NULL = pixels 0 .. N-1; W the frame's width (n_pix = H W).
 *   code 0 -> 0 (no measurement),  code 65535 -> +inf (known empty),  else
 *   target[k] = ((float)code * unit) * sqrt((x x + y y) + 1),   x = ((i + 0.5) - cx) / fx,  y = ((j + 0.5) - cy) / fy,  (i, j) = (pix % W, pix / W)
 * -- the RAY DISTANCE of the pixel: its z-depth times the length of the direction get_rays forms for it before normalising, with
 * unit = integer_depth_scale * opt.scale (one float).  Every operation is one fp32 operation.  An id outside [0, n_pix) reads nothing
 * and gives 0.  target float [N]. */
NGP_API int ngp_train_depth_targets(const uint16_t* store, uint64_t frame_base, uint32_t n_pix, uint32_t W, const int64_t* inds, uint32_t N,
                            float fx, float fy, float cx, float cy, float unit, float* target, ngp_stream_t stream);

/* MSELoss(reduction='none')(pred, gt).mean(-1) and its mean over the rays (utils.py:450,480) in one launch (two above 16384 rays):
 * pred [N,3] of pred_dtype 0 = f32 / 1 = f16, gt float [N,3] -> per_ray float [N] = ((d0^2 + d1^2) + d2^2) / 3, *mean (device float).
 * The mean is a fixed-order sum -- 64-ray groups by a butterfly, the groups in double, strided by 64 and by the same butterfly --
 * that depends on N alone: no float atomics, the same bits on every call and for either launch shape.
 * error_row (float [map_len], may be NULL) with inds_coarse (int64 [N]): error_row[inds_coarse[i]] = 0.1 * error_row[inds_coarse[i]] +
 * 0.9 * per_ray[i], the error-map update of utils.py:474-475 (the OLD value weighted by 0.1).  PRECONDITION: the ids are distinct, as
 * torch.multinomial(..., replacement=False) draws them (two rays on one entry would race); an id outside [0, map_len) is skipped.
 * workspace: ngp_photo_loss_workspace(N) bytes (0 up to 16384 rays: NULL is fine). */
NGP_API size_t ngp_photo_loss_workspace(uint32_t N);
NGP_API int ngp_photo_loss_forward(const void* pred, int pred_dtype, const float* gt, uint32_t N, float* per_ray, float* mean, float* error_row,
                           uint32_t map_len, const int64_t* inds_coarse, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
/* grad_pred [N,3] (pred's dtype) = *g * 2 * (pred - gt) / (3 N); g is a DEVICE float (the GradScaler's scaled seed gradient never
 * comes back to the host). */
NGP_API int ngp_photo_loss_backward(const void* pred, int pred_dtype, const float* gt, uint32_t N, const float* g, void* grad_pred,
                            ngp_stream_t stream);

/* ---------------- distortion regulariser (loss.py:29-76 eff_distloss; mip-NeRF 360 eq. 15 in its O(n) form) ---------------- */

/* Per ray of a table rays int32 [N,3] = (index, offset, count), with per-sample weight w_i, position m_i (non-decreasing) and width
 * delta_i at the packed rows offset .. offset + count - 1:
 *   L_ray = 2 sum_i w_i (m_i Wpre_i - WMpre_i) + (1/3) sum_i w_i^2 delta_i,   Wpre_i = sum_{j<i} w_j,  WMpre_i = sum_{j<i} w_j m_j
 *         ( = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i for sorted m; for unsorted m it is still the expression above,
 *           which is what the reference evaluates)
 *   g_i   = dL_ray / dw_i = 2 (m_i (Wpre_i - Wsuf_i) + (WMsuf_i - WMpre_i)) + (2/3) delta_i w_i
 * loss_rays float [N]: L_ray at slot `index`;  *loss (device float) = (sum of loss_rays) / N, N counting every row of the table;
 * totals float [N,2]: (sum w, sum w m) of the ray at slot `index`, which the backward call reads.  The index column must hold every
 * slot 0 .. N-1 once (as march_rays_train writes it; a row with index >= N is ignored, its slot is not written).  One wave per ray,
 * prefix sums by wave scans; the mean is the fixed-order sum of ngp_photo_loss_forward over the SLOTS.  No atomics: the same bits on
 * every call and for every order of the table's rows.  workspace: ngp_distortion_workspace(N) bytes (0 up to 16384 rays).
 *
 * ngp_distortion_train_*: the packed layout of march_rays_train, sigmas float [M], deltas float [M,2] = (dt, gap), 8-byte aligned:
 *   alpha_i = 1 - exp(-sigma_i dt_i),  T_0 = 1,  T_{i+1} = T_i (1 - alpha_i),  w_i = alpha_i T_i,
 *   m_i = scale * sum_{k<=i} gap_k  (the t that composite_rays_train integrates into depth),  delta_i = scale * dt_i,
 * scale float [N] read at `index` (NULL = 1; the renderer passes 1 / (far - near)).  The ray ends behind the first sample with
 * T_{i+1} < 1e-4, that sample included (the forward rule of composite_rays_train); a ray with count == 0 or offset + count >= M is
 * dropped as composite_rays_train drops it: loss 0, no gradient.  T is the running product of the (1 - alpha).
 *   grad_sigmas[offset + k] = (*grad_loss / N) dt_k (g_k T_{k+1} - sum_{i>k} g_i w_i)     for every live sample k
 * -- the exact derivative, the sample that stops the ray included (composite_rays_train_backward writes none for that one).  Rows of
 * dead samples, of dropped rays and of no ray are NOT written: hand in zeros.  grad_loss is a device float.
 *
 * ngp_distortion_forward / _backward: the same scans on given w, m float [M] and interval (float [M], or NULL: interval_scalar for
 * every sample); every sample of a ray is live, and a ray is dropped only when count == 0 or offset + count > M (a dense [B,T] input
 * is the table (i, i T, T) with M = B T).  grad_w[offset + k] = (*grad_loss / N) g_k; other rows are not written. */
NGP_API size_t ngp_distortion_workspace(uint32_t N);
NGP_API int ngp_distortion_train_forward(const float* sigmas, const float* deltas, const int32_t* rays, const float* scale, uint32_t M,
                                 uint32_t N, float* loss_rays, float* totals, float* loss, void* workspace, size_t workspace_bytes,
                                 ngp_stream_t stream);
NGP_API int ngp_distortion_train_backward(const float* grad_loss, const float* sigmas, const float* deltas, const int32_t* rays,
                                  const float* scale, const float* totals, uint32_t M, uint32_t N, float* grad_sigmas,
                                  ngp_stream_t stream);
NGP_API int ngp_distortion_forward(const float* w, const float* m, const float* interval, float interval_scalar, const int32_t* rays,
                           uint32_t M, uint32_t N, float* loss_rays, float* totals, float* loss, void* workspace,
                           size_t workspace_bytes, ngp_stream_t stream);
NGP_API int ngp_distortion_backward(const float* grad_loss, const float* w, const float* m, const float* interval, float interval_scalar,
                            const int32_t* rays, const float* totals, uint32_t M, uint32_t N, float* grad_w, ngp_stream_t stream);

/* ---------------- depth supervision (DESIGN.md "Depth supervision") ---------------- */

/* Per ray of a table rays int32 [N,3] = (index, offset, count) over packed sigmas [M] and deltas [M,2] = (dt, gap), with the composite
 * rule ngp_distortion_train_* uses: alpha_i = 1 - exp(-sigma_i dt_i), T_0 = 1, T_{i+1} = T_i (1 - alpha_i), w_i = alpha_i T_i,
 * t_i = sum_{k<=i} gap_k.  The ray ends behind the first sample with T_{i+1} < 1e-4, that sample included.  A ray with
 * offset + count >= M is dropped.  Each ray has a target z = target[index], a ray distance in the units of t, and a per-ray
 * scale[index] (NULL = 1; the renderer passes 1 / (far - near), as it does for the distortion term).
 *   z == 0, or NaN, or negative: no measurement.  L_ray = 0, and every gradient row of the ray is left at the zeros handed in.
 *   0 < z < +inf: a surface at z.   d = sum_live w_i t_i,   A = sum_{live, t_i < z - margin} w_i,
 *                                   L_ray = a (scale (d - z))^2 + b A
 *   z == +inf: known empty ray.     A = sum_live w_i,   L_ray = b A
 * A is the opacity the ray has accumulated before the margin in front of the surface, 1 - T there: bounded by 1 and independent of how
 * densely the ray was sampled, which is why it is linear in w and not a sum of w_i^2.
 *   g_i = dL_ray / dw_i = 2 a scale^2 (d - z) t_i + b [t_i < z - margin]
 *   dL_ray / dsigma_i = dt_i (T_{i+1} g_i - sum_{k>i, live} g_k w_k)        exact, the sample that stops the ray included
 * *loss (device float) = sum over the slots of L_ray / N, over all N slots and not over the valid ones, by the fixed-order mean of
 * ngp_photo_loss_forward.  a = weight_depth, b = weight_free and margin are host floats.
 * loss_rays float [N]: L_ray at slot `index`;  parts float [N,2]: (d, A) at slot `index` (0, 0 for a ray without a measurement or a
 * dropped one), which the backward call reads: its suffix sums are a total minus a prefix, the total being
 * 2 a scale^2 (d - z) d + b A.  A row with index >= N is ignored; target and scale are read at a valid index only; the drop rule is
 * applied before any row is read.  grad_sigmas[offset + k] = (*grad_loss / N) dL_ray / dsigma_k for live samples k; rows of dead
 * samples, of rays that take no part and of no ray are NOT written: hand in zeros.  grad_loss is a device float.
 * One wave per ray, prefix sums by wave scans, no LDS and no atomics: the same bits on every call and for every order of the table's
 * rows.  workspace: ngp_depth_loss_workspace(N) bytes (0 up to 16384 rays).
 *
 * ngp_depth_loss_forward / _backward: the same on given w, t float [M]; every sample of a ray is live and a ray is dropped only when
 * count == 0 or offset + count > M (a dense [B,T] input is the table (i, i T, T) with M = B T).
 * grad_w[offset + k] = (*grad_loss / N) g_k; other rows are not written. */
NGP_API size_t ngp_depth_loss_workspace(uint32_t N);
NGP_API int ngp_depth_loss_train_forward(const float* sigmas, const float* deltas, const int32_t* rays, const float* target, const float* scale,
                                 float margin, float weight_depth, float weight_free, uint32_t M, uint32_t N, float* loss_rays,
                                 float* parts, float* loss, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
NGP_API int ngp_depth_loss_train_backward(const float* grad_loss, const float* sigmas, const float* deltas, const int32_t* rays,
                                  const float* target, const float* scale, float margin, float weight_depth, float weight_free,
                                  const float* parts, uint32_t M, uint32_t N, float* grad_sigmas, ngp_stream_t stream);
NGP_API int ngp_depth_loss_forward(const float* w, const float* t, const int32_t* rays, const float* target, const float* scale, float margin,
                           float weight_depth, float weight_free, uint32_t M, uint32_t N, float* loss_rays, float* parts, float* loss,
                           void* workspace, size_t workspace_bytes, ngp_stream_t stream);
NGP_API int ngp_depth_loss_backward(const float* grad_loss, const float* w, const float* t, const int32_t* rays, const float* target,
                            const float* scale, float margin, float weight_depth, float weight_free, const float* parts, uint32_t M,
                            uint32_t N, float* grad_w, ngp_stream_t stream);

/* ---------------- image quality (uncertainty/evaluation/image_metrics.py:79-135; nerf/utils.py PSNRMeter) ---------------- */

/* The sums behind PSNR and SSIM of B three-channel frames in one pass.  pred and target are float images addressed by ELEMENT strides
 * (the same for both): element (b, c, y, x) is at b * stride_b + c * stride_c + y * stride_y + x * stride_x, so the Trainer's
 * [B,H,W,3] and the reference modules' [B,3,H,W] are read in place (strides >= 0).  mask: float [B,H,W] of weights, or NULL = all one.
 * The SSIM map is torchmetrics' structural_similarity_index_measure(data_range, return_full_image=True): window g (x) g with
 * g[i] = exp(-(i / 1.5)^2 / 2) / sum, i = -5..5; both images reflect-padded by 5 (index -k -> k, H-1+k -> H-1-k); the windowed sums of
 * p, t, p^2, t^2, p t give mu_p, mu_t, var_p = max(E[p^2] - mu_p^2, 0) (likewise var_t), cov = E[p t] - mu_p mu_t (not clamped);
 * c1 = (0.01 range)^2, c2 = (0.03 range)^2;  ssim = ((2 mu_p mu_t + c1)(2 cov + c2)) / ((mu_p^2 + mu_t^2 + c1)(var_p + var_t + c2)).
 * The window sums and the formula are evaluated in double.  ssim_map (float [B,H,W], may be NULL) receives the mean over the channels.
 * stats (device, [B,8] doubles), per image:
 *   [0] sum mask * ssim (channel mean)   [1] sum mask   [2..4] sum mask * (pred - target)^2 per channel   [5] H * W   [6] [7] 0
 * Partial sums per workgroup go to the CALLER's workspace (ngp_image_quality_workspace(B, H, W) bytes, 8-byte aligned; NGP_EWORKSPACE
 * when smaller) and are added in double in a fixed order by a second small launch: no atomics, no state between calls -- the same bits
 * on every call, per image independent of the rest of the batch, and calls on different streams with their own workspaces do not
 * interact.  H, W in [6, 32768] (torch's reflect pad needs more than 5), 1 <= B <= 65535, data_range > 0: NGP_EINVAL otherwise,
 * nothing launched (the workspace size of a refused shape is 0). */
NGP_API size_t ngp_image_quality_workspace(uint32_t B, uint32_t H, uint32_t W);
NGP_API int ngp_image_quality(const float* pred, const float* target, const float* mask, uint32_t B, uint32_t H, uint32_t W,
                      int64_t stride_b, int64_t stride_c, int64_t stride_y, int64_t stride_x, float data_range, float* ssim_map,
                      double* stats, void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* ---------------- keypoint detection (nav/features.py) ---------------- */
/* SIFT's detection stage with cv2.SIFT_create()'s defaults (3 layers per octave, contrast 0.04, edge 10, sigma 1.6, first octave -1)
 * on an RGB uint8 frame [H][W][3], and the state estimator's interest mask (nav/estimator_helpers.py:95-107).  Outputs, both uint8
 * [W][H] (x-major, the reference's interest_regions[x, y]): points = 1 at the truncated position of every accepted keypoint; mask =
 * points dilated with a kernel_size^2 box dil_iter times (cv2.dilate: anchor at the centre, pixels outside do not contribute).
 * count [1] device = number of accepted keypoints (before deduplication; 0 is the estimator's failure branch).  H, W in [8, 16384]
 * and 20 H W < 2^32 (the element counts of octave 0's DoG planes are 32-bit).
 * The workspace holds the Gaussian and DoG pyramids: ngp_sift_workspace(H, W) bytes (0: unsupported size); octave o's layer
 * `index` (0..5 Gaussian, 6..10 DoG, float [rows_o][cols_o]) starts at byte ngp_sift_layer_offset(H, W, o, index) and stays
 * valid until the workspace is reused; ngp_sift_octaves(H, W) octaves, rows_0 = 2 H, cols_0 = 2 W, halved (floor) per octave. */
NGP_API size_t ngp_sift_workspace(uint32_t H, uint32_t W);
NGP_API size_t ngp_sift_layer_offset(uint32_t H, uint32_t W, int octave, int index);
NGP_API int ngp_sift_octaves(uint32_t H, uint32_t W);
NGP_API int ngp_sift_interest_mask(const uint8_t* rgb, uint32_t H, uint32_t W, uint32_t kernel_size, uint32_t dil_iter, uint8_t* points,
                                   uint8_t* mask, uint32_t* count, void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* Diagnostics.  ngp_debug_set_stamps / ngp_debug_set_sample_hash / ngp_debug_disable_march_queue set the PROCESS DEFAULT;
 * ngp_render_ctx_set_debug(ctx, 1, flags, stamps, sample_hash) gives one context its own state (enable = 0: back to the default);
 * `flags` is a word of enum ngp_debug_flag below.
 * A render call snapshots the state that applies to it once, at its start: concurrent calls on other threads / streams are not
 * affected by a change made while they run.
 * When a device buffer of >= 16 uint64 is set, k_render_iter adds per-phase wave-cycle sums
 * (s_memtime deltas: [0] march, [1] encode+MLP tiles, [2] composite, [3] compaction+barrier; [4..6] march lane statistics; [8] encode + sigma net, [9] colour net, [10] tiles, [11] samples in them).  NULL (default) = no
 * stamp instruction executes. */
NGP_API int ngp_debug_set_stamps(unsigned long long* device_buf);
/* Diagnostics: uint32[N] device buffer receiving, per ray, an FNV-1a hash over the bit patterns of (dt, deltas[1]) of every
 * sample the fused renderer marched, in order (NULL = off).  Lets a test prove the fused path's sample sequence equal to
 * march_rays' bit for bit. */
NGP_API int ngp_debug_set_sample_hash(uint32_t* device_buf);
/* The debug flag word of the fused render loop (ngp_render_rays): every bit switches one scheduling device off.  Results do not
 * depend on any of them (the tests compare images and sample hashes bit for bit across them).  The numeric values are frozen. */
enum ngp_debug_flag {
    NGP_DBG_NO_BLOCK_JUMP = 1 << 0,        /* no one-step exit from empty 4x4x4 blocks (Dda::jump_block) */
    NGP_DBG_NO_COARSE = 1 << 1,            /* no coarse occupancy filter: plain probes (and then no linear re-layout, no slow-ray grouping) */
    NGP_DBG_NO_SLOW_SORT = 1 << 2,         /* no grouping of the slow rays at the end of the alive list */
    NGP_DBG_NO_LIN = 1 << 3,               /* no linear (x-fastest) re-layout of the occupancy bits */
    NGP_DBG_ONE_ITER_PER_LAUNCH = 1 << 8,  /* no launch covers several reference iterations */
    NGP_DBG_NO_TILES = 1 << 13,            /* the frame-width hint is ignored: no 4x4-pixel tiles in the alive list */
    NGP_DBG_NO_PRE_VERDICT = 1 << 14,      /* every multi-iteration launch runs as planned (no cut before the network from the march's counts) */
    NGP_DBG_WIDE_ITEMS = 1 << 15,          /* the work items of k_render_iter stay 64 list entries wide */
    NGP_DBG_REPLAY_ONE_ITER = 1 << 16,     /* a launch that failed its verification is replayed as one iteration, not as its verified prefix */
    NGP_DBG_LANE_MARCH = 1 << 17,          /* k_march_ahead marches a lane per ray always (never a wave per ray) */
    NGP_DBG_PROBE_PER_SAMPLE = 1 << 18,    /* k_march_ahead probes the occupancy bits for every sample (no runs inside an occupied cell) */
    NGP_DBG_ALL = 0x7E10F                  /* every bit above; a flag word with any other bit set is refused with NGP_EINVAL */
};
/* Sets the WHOLE flag word of the process default (the name is historic: the first flag switched a march queue off). */
NGP_API int ngp_debug_disable_march_queue(int flags);
/* Diagnostics: the 32 hash-grid features of xyzs [M,3] (positions in [-bound, bound]) exactly as the fused kernels' gather forms them
 * -> features [M,32] fp16 in the operator's order (2 * level + channel).  operator_rounding = 0: the fused kernels' arithmetic (fp32
 * accumulation of the 8 corners, one rounding); 1: the grid_encode operator's (c10::Half product and running sum,
 * gridencoder.cu:169-172) through the same gather -- bit-identical to ngp_grid_encode_forward, which is how the default's
 * deviation from the reference arithmetic is measured (tests/test_render_gpu.py). */
/* With an NGP_PREC_F32 model `features` is float [M,32] and operator_rounding is ignored (one arithmetic: the operator's fmaf chain). */
NGP_API int ngp_debug_fused_features(const ngp_model* model, const float* xyzs, uint32_t M, int operator_rounding, uint16_t* features,
                             ngp_stream_t stream);
/* Diagnostics of ngp_render_uniform_backward: float [N][T][4] device buffer receiving, per sample, sigma, the transmittance before
 * it, dL/dw and dL/dsigma (NULL = off; process-wide, single-threaded use). */
NGP_API int ngp_debug_set_grad_dump(float* device_buf);
NGP_API int ngp_render_ctx_set_debug(ngp_render_ctx* ctx, int enable, int flags, unsigned long long* stamps, uint32_t* sample_hash);

/* ---------------- per-kernel device timing (bench.py roofline leg) ---------------- */
/* When enabled, selected kernels are bracketed by hipEvents on their own stream.
 * ngp_prof_read synchronises the recorded events and returns accumulated milliseconds
 * and launch count for `name`; returns NGP_EINVAL for unknown names. */
NGP_API int ngp_prof_enable(int on);
NGP_API int ngp_prof_reset(void);
NGP_API int ngp_prof_read(const char* name, double* total_ms, uint64_t* launches, double* units);

#ifdef __cplusplus
}
#endif
#endif /* NGP_HIP_H */
