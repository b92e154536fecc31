// Host functions that one translation unit of liburso_hip.so defines and another calls: declared here once and included by both sides,
// so that a definition is compiled against its declaration.  Internal to the library; the C ABI is include/ursonet_hip.h.
// Convention: urso_X_fits() says whether kernel family X takes a layer, urso_X_launch() enqueues it and returns URSO_OK or an error,
// urso_X_splits() is the number of fp32 partials its weight gradient writes (what the caller sizes the workspace for); a urso_X_try*()
// returns 1 after launching, 0 when the layer does not take the kernel (the caller's own then serves it), < 0 on a launch error.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- forward / data-gradient convolutions (dispatch: conv_igemm.hip urso_conv_igemm_ex)
// conv_pw.hip: DMA-staged implicit GEMM; it offers pointwise layers to conv_pwx.hip first
int urso_pw_launch(const urso_conv_geom* g, int dt, int conv, int dhs, int dws, int relu,
                   const void* src, const void* wgt, const float* bias, const void* add, const void* mask, void* dst,
                   uint32_t src_bytes, uint32_t wgt_bytes, uint32_t dst_bytes, int mask_bits, void* bits_out, int add_src, hipStream_t st);
int urso_pwx_try(const urso_conv_geom* g, int dt, int relu, const void* src, const void* wgt, const float* bias, const void* add,
                 const void* mask, void* dst, uint32_t src_bytes, uint32_t wgt_bytes, uint32_t dst_bytes, int mask_bits, void* bits_out,
                 hipStream_t st);
// conv_pair.hip: the single c -> 4c pointwise layers on the pair kernel's pipeline
bool urso_pair_single_fits(const urso_conv_geom* g, int dt, int flags, const void* add, const void* mask);
int urso_pair_single_launch(const urso_conv_geom* g, int dt, int flags, const void* src, const void* wgt, const float* bias, const void* add,
                            const void* mask_bits, void* dst, void* bits_out, hipStream_t st);
// conv_stem.hip: the packed 7x7 stem
bool urso_stem_fits(const urso_conv_geom* g, int dt, int flags, const void* add, const void* mask);
int urso_stem_launch(const urso_conv_geom* g, int dt, int relu, const void* src, const void* wgt, const float* bias, void* dst, hipStream_t st);
// conv_c3.hip: 3x3 layers with the filter in registers
bool urso_c3_fits(const urso_conv_geom* g, int dt, int flags, const void* add);
int urso_c3_launch(const urso_conv_geom* g, int dt, int relu, const void* src, const void* wgt, const float* bias, const void* mask,
                   void* dst, hipStream_t st);
// conv_halo.hip: halo-tile 3x3 layers; conv_halo2.hip: whole tiles of a per-layer shape, which urso_hconv_launch tries first
// (urso_hconv2_pick: 10 * MI + NJ of the shape it would run the layer on, 0 = conv_halo.hip keeps it)
bool urso_hconv_fits(const urso_conv_geom* g, int dt, int flags, const void* add);
int urso_hconv_launch(const urso_conv_geom* g, int dt, int relu, const void* src, const void* wgt, const float* bias, const void* add,
                      const void* mask, void* dst, uint32_t src_bytes, uint32_t wgt_bytes, uint32_t dst_bytes, void* ws, size_t ws_bytes,
                      hipStream_t st);
size_t urso_hconv_ws_bytes();
int urso_hconv2_pick(const urso_conv_geom* g, bool has_ws);
int urso_hconv2_try_launch(const urso_conv_geom* g, int dt, int relu, const void* src, const void* wgt, const float* bias, const void* mask,
                           void* dst, uint32_t src_bytes, uint32_t wgt_bytes, uint32_t dst_bytes, void* ws, bool has_ws, hipStream_t st);
// conv_bneck.hip: bottleneck_layer (3x3 / stride 2, <= 32 filters), forward and data gradient
bool urso_bneck_fwd_fits(const urso_conv_geom* g, int dt, int flags, const void* add, const void* mask);
int urso_bneck_fwd_launch(const urso_conv_geom* g, int dt, int flags, const void* src, const void* wgt, const float* bias, void* dst, hipStream_t st);
bool urso_bneck_dgrad_fits(const urso_conv_geom* g, int dt, int flags, const void* add, const void* mask);
int urso_bneck_dgrad_launch(const urso_conv_geom* g, int dt, int flags, const void* dz, const void* wd, const void* mask, void* dst, hipStream_t st);
// conv_dense.hip: skinny GEMM of the Dense heads
bool urso_dense_fits(const urso_conv_geom* g, int dt, int flags, int pointwise, long long M);
int urso_dense_launch(const urso_conv_geom* g, int dt, int flags, const void* src, const void* wgt, const float* bias, const void* add,
                      const void* mask, void* dst, uint32_t src_bytes, uint32_t wgt_bytes, uint32_t dst_bytes, hipStream_t st);

// ---------------------------------------------------------------- weight gradients (dispatch: conv_wgrad.hip)
// conv_c3g.hip: the 64-channel 3x3 layers keep the whole gradient in registers (one partial per block)
bool urso_c3g_fits(const urso_conv_geom* g, int dt);
int urso_c3g_splits(const urso_conv_geom* g);
int urso_c3g_launch(const urso_conv_geom* g, int dt, const void* x, const void* dz, float* part, float* colpart, size_t part_stride, hipStream_t st);
// conv_hwgrad.hip: the same scheme for the 3x3 layers with >= 128 channels, one (64-channel, 64-filter) group of the gradient per block
bool urso_hwg_fits(const urso_conv_geom* g, int dt);
int urso_hwg_splits(const urso_conv_geom* g);
int urso_hwg_launch(const urso_conv_geom* g, int dt, const void* x, const void* dz, float* part, float* colpart, size_t part_stride, hipStream_t st);
bool urso_hwg_pair_splits(const urso_conv_geom* g0, const urso_conv_geom* g1, int dt, int* s0, int* s1);
int urso_hwg_launch2(const urso_conv_geom* g0, const urso_conv_geom* g1, int dt, const void* x0, const void* dz0, float* part0, float* colpart0,
                     const void* x1, const void* dz1, float* part1, float* colpart1, hipStream_t st);
// conv_stemw.hip: the packed 7x7 stem has a kernel of its own (one partial per block)
bool urso_stemw_fits(const urso_conv_geom* g, int dt);
int urso_stemw_splits(const urso_conv_geom* g, bool pooled);
int urso_stemw_launch(const urso_conv_geom* g, int dt, const void* x, const void* dz, const void* dpool, const uint8_t* am,
                      float* part, float* colpart, size_t part_stride, hipStream_t st);
// conv_wgrad.hip: the batched split reduction, one phase of prep.hip's urso_param_batch_run
void urso_reduce_partials_batch_launch(const urso_param_desc* descs_d, const int32_t* blockmap_d, int nblocks, hipStream_t st);
