/*
 * sam2hip.h -- C ABI of libsam2hip.so, the MI355X (gfx950) compute path of the
 * SAM2 video fine-tuning step (SAM2LightningModule.training_step,
 * reference sam2_video/training/trainer.py:256-289).
 *
 * Every entry point takes raw device pointers, int64 element strides, a dtype
 * tag, scalar parameters and the hipStream_t to launch on.  Nothing allocates
 * (workspaces are passed in), nothing synchronises, and every call returns a
 * hipError_t value (0 = success).  Element strides are in elements, not bytes.
 * Tensors are owned by the caller (the Python host package uses PyTorch's
 * caching allocator).  The library keeps no per-thread state; forward launches
 * come from the Python thread, backward launches from the autograd worker.
 *
 * Each declaration names the reference operation it replaces (file:line in the
 * reference repository, sam2_video/... paths; the modeling files are the
 * vendored SAM2.1 sources under sam2_video/model/modeling/).
 */
#ifndef SAM2HIP_H
#define SAM2HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Same definition as hip_runtime_api.h, so the two headers can be combined. */
typedef struct ihipStream_t* hipStream_t;

/* dtype tags (`dt` arguments) */
enum { S2H_F32 = 0, S2H_BF16 = 1 };
/* fused activations (`act` arguments) */
enum { S2H_ACT_NONE = 0, S2H_ACT_RELU = 1, S2H_ACT_GELU = 2, S2H_ACT_SIGMOID = 3 };

/* ---------------------------------------------------------------- library */
/* ABI version (1). */
int s2h_version(void);
/* Bind a device-resident uint64 RNG offset (NULL unbinds).  Every dropout site
 * (s2h_gemm epilogue, s2h_attn_fwd/bwd, s2h_dropout) folds its current value into
 * the seed it was launched with, at kernel start: a captured HIP graph of the step
 * replays with fresh dropout masks (memory_attention.py:40-48, transformer.py:304-306
 * dropout_p) once the host advances the offset between replays; 0 = unchanged seed. */
int s2h_rng_bind(const void* dev_u64);
/* In-library launch profiler: `cap` > 0 pre-creates `cap` HIP event pairs and
 * brackets every launch of a selected kind on the stream it is launched on; 0 disables. */
int s2h_prof_enable(int cap);
/* kinds recorded: bit 1 attention forward, 2 attention backward, 4 GEMM, 8 trace markers (default 1) */
int s2h_prof_select(int mask);
int s2h_prof_reset(void);
int s2h_prof_count(void);
/* Copies up to `max` records: ms[i] (event elapsed time) and meta[6*i..] = (kind, shape):
 * attention (1, 2): (batch*heads, Lq, Lk, head_dim, element size);
 * GEMM (4): (batch, M, N, K, 2*A_kcontig + B_kcontig + 4*bf16).  Synchronises the events. */
int s2h_prof_read(int max, float* ms, int64_t* meta);
/* tags[i] = the kernel record i launched (0 = not tagged): GEMM tilings as
 * BM | BN << 10 | WGM << 20 | WGN << 24 | NS << 28 | (BK / 32) << 32 | A_kcontig << 36 |
 * B_kcontig << 37 | register_staged << 38 | mx_fp8 << 39 | a_in_registers << 40 |
 * deterministic_wgrad << 41 | ffn_bwd_dgrad << 42 | ffn_fwd << 43 -- the template arguments of the kernel rocprofv3 names (bench.py: the
 * roofline's dominant kernel). */
int s2h_prof_read_tags(int max, int64_t* tags);
/* Launches a one-lane no-op kernel (s2h_trace_marker_kernel) on `st`: brackets a region of a
 * rocprofv3 kernel trace (bench.py's timed steps, tools/step_profile.py). */
int s2h_trace_marker(int tag, hipStream_t st);

/* ---------------------------------------------------------------- GEMM
 * C[b](m,n) = act(alpha * sum_k A[b](m,k) B[b](k,n) + bias) * cscale[n], dropout(p, seed),
 *             + R[b](m,n) + beta * C[b](m,n)
 * (dropout element index drop_idx0 + (b*M + m)*N + n: a launch over frame f of a frame-stacked
 *  activation passes f*M*N so the frame-batched backward regenerates the same mask)
 * A addressed as A[m*lda_m + k*lda_k] (one of lda_m, lda_k must be 1), B as
 * B[k*ldb_k + n*ldb_n] (one of ldb_k, ldb_n must be 1), batch strides sA/sB/sC.
 * dt_ab: S2H_F32 (fp32 MFMA, parity mode; dt_c must be F32) or S2H_BF16 (bf16 MFMA,
 * fp32 accumulate; dt_c BF16 or F32).  bias_mode 1 = per column, 2 = per row.
 * aux_mode 1 stores the pre-activation into X; 2 multiplies by act'(X) (the
 * activation gradient of the layer that produced X) instead of applying act.
 * Element types: R and X have the A / B element type dt_ab, NOT the output type dt_c -- a bf16 GEMM
 * with an fp32 C reads R and reads / writes X as bf16, the fp32 GEMM as fp32; bias and cscale are fp32.
 * Order per element: v = alpha * acc + bias; X = v (aux_mode 1); v = act(v) or v * act'(X) (aux_mode 2);
 * v *= cscale[n]; dropout; + R; + beta * C; one rounding to dt_c.
 * Dropout: counter hash of (seed folded with the bound RNG offset, element index), csrc/common.h; the
 * drop probability is quantised to 1/65536: an element is dropped with probability
 * floor(drop_p * 65536) / 65536 (kept values are still scaled by 1 / (1 - drop_p)).  The same holds at
 * every dropout site of this header (s2h_dropout, s2h_act_dropout_bwd, s2h_linear_add_ln, s2h_ffn_fwd,
 * attention).
 * Replaces every nn.Linear / 1x1 nn.Conv2d / im2col conv / matmul on the path:
 *   hieradet.py:56-81 (qkv, proj), :140 (dim-change proj), sam2_utils.py:112-139 (MLP),
 *   transformer.py:230-243, 275-311 (q/k/v/out proj), memory_attention.py:58-99 (FFN),
 *   image_encoder.py:79 (FPN lateral 1x1), mask_decoder.py:66-81 (ConvT 2x2 / conv_s0/s1),
 *   utils.py:85 (PatchEmbed 7x7/4 conv), memory_encoder.py:43-156 (mask downsampler,
 *   CXBlock pwconv, pix_feat_proj, out_proj), mask_decoder.py:168-245 (hypernetwork
 *   product), hieradet.py:273-281 (bicubic pos-embed resize as two GEMMs),
 *   and their autograd backward (dgrad / wgrad). */
int s2h_gemm(int dt_ab, int dt_c, int batch, int M, int N, int K,
             const void* A, int64_t lda_m, int64_t lda_k, int64_t sA,
             const void* B, int64_t ldb_k, int64_t ldb_n, int64_t sB,
             void* C, int64_t ldc, int64_t sC,
             const float* bias, int bias_mode,
             const void* R, int64_t ldr, int64_t sR,
             void* X, int64_t ldx, int64_t sX, int aux_mode,
             const float* cscale, float drop_p, uint64_t seed, uint64_t drop_idx0,
             float alpha, float beta, int act, hipStream_t stream);

/* A/B switch (tests, benchmarks) for the bf16 GEMM tiling; returns the previous setting.
 * 0 = automatic by shape, -1 = register-staged kernel, LDS-DMA tilings: 1 = 64x64,
 * 2 = 128x128, 3 = 128x128 with a 3-deep ring, 4 = 256x128, 5 = 256x256, 6 = 128x256,
 * 7 = 128x64, 8 = 64x128, 9 = 64x64 with a 3-deep ring, 10 = 64x64 32-deep 4-deep ring,
 * 11 / 12 / 13 = 128x64 32-deep 3- / 4-deep ring and 64-deep 3-deep ring, 14 / 15 = 256x128 on 4 waves
 * (32-deep 3-deep ring / 64-deep 2-deep), 16 = 128x128 32-deep 3-deep ring, 17 = 256x64 on 4 waves;
 * bits 8+ are measurement-only ablations of the LDS-DMA kernel (results are wrong):
 * 256 = skip the epilogue stores, 512 = skip the MFMAs. */
int s2h_gemm_config(int cfg);

/* A/B knob (tests, benchmarks): workgroups a split-K weight-gradient GEMM aims at (default 768;
 * t <= 0 leaves it unchanged); returns the previous value. */
int s2h_gemm_split_target(int t);

/* A/B knob (tests, benchmarks): tiling of the GEMMs with M <= 128 rows (0 = automatic, values as
 * s2h_gemm_config); returns the previous setting. */
int s2h_gemm_tiny_config(int cfg);
/* A/B knob: the bf16-output GEMMs on 4 x 1 wave grids (whole 64-column rows per wave) instead of
 * 2 x 2 (1: all, the default; 2: only N >= 768; 0: off); results are bit-identical.  Returns the
 * previous mode. */
int s2h_gemm_w41(int mode);
/* A/B knob (round 6): tiling (values as s2h_gemm_config, 0 = the shape rules) of one class of
 * bf16-output GEMMs with M > 128 -- class 0: K >= 1024 and N <= 512; 1: K <= 256, N <= 256 and
 * M >= 8192; 2: K <= 512 and N >= 768; 3: 256 < K < 1024 and N <= 512; 4 / 5: K < 256 not a multiple
 * of 64 with M >= 65536 / with M < 65536 and K >= 128.  Returns the previous setting (-1: no such class). */
int s2h_gemm_class_config(int cls, int cfg);
/* A/B knob (round 6): bf16-output GEMMs with M <= 128, K >= 1024 and at most 16 64 x 64 output tiles as
 * one split-K fp32 launch into the weight-gradient workspace + one fixed-order reduce running the
 * GEMM epilogue (1: on; 0: the one-launch tiling, the default -- measured step-neutral); mode < 0 only queries.  Returns the
 * previous mode. */
int s2h_gemm_tiny_splitk(int mode);
/* A/B knob: GEMMs with a short K that is not a multiple of 64 (K < 256, K-contiguous A, bf16 output)
 * on the A-in-registers tiling (1: on, the default; 0: off); results are bit-identical.  Returns the
 * previous mode. */
int s2h_gemm_areg(int mode);
/* flash forward: 16-query sets per wave (1 or 2; bits 0-3 V-fold launches, 4-7 plain launches with
   head dim <= 128); returns the previous mode, < 0 only queries.  Same results either way. */
int s2h_flash_fwd_sets(int mode);

/* Weight and bias gradient of a Linear layer (autograd of nn.Linear, e.g. hieradet.py:56-81,
 * memory_attention.py:58-99): dw[N, K] (+)= dy[rows, N]^T x[rows, K] (dw row stride lddw),
 * db[N] (+)= sum over rows of dy (db may be NULL); `accumulate` 0 overwrites both.
 * bf16 dy/x: one launch, the bias gradient summed from the GEMM's staged dy tiles. */
int s2h_linear_wgrad(int dt, int64_t rows, int N, int K, const void* dy, int64_t lddy, const void* x,
                     int64_t ldx, float* dw, int64_t lddw, float* db, int accumulate, hipStream_t stream);

/* Workspace of the deterministic weight-gradient GEMM (round 5, csrc/gemm_wgrad.hip): bf16 GEMMs with
 * an fp32 output, both operands row-contiguous over a reduction of >= kmin rows (the Linear weight
 * gradients of s2h_linear_wgrad / s2h_gemm, e.g. memory_attention.py:97's FFN over 93184 rows) run on
 * 256 x 256-class tiles, write per-split fp32 partial tiles here and add them in fixed split order:
 * the gradient arena is bit-identical from run to run (the split-K path added with fp32 atomics).
 * ws: device memory of `bytes` owned by the caller (NULL: none, the atomic path runs); launches
 * using it must be stream-ordered.  kmin 0 turns the kernel off, -1 keeps the current value (4096).
 * Returns 0. */
int s2h_wgrad_workspace(void* ws, int64_t bytes, int kmin);
/* Measurement knob (tools/wgrad_bench.py): force that kernel's tile (0 = 256x256, 1 = 256x128,
 * 2 = 128x256, 3 = 128x128, 4 = 256x64, 5 = 64x256; -1 = its cost model) and split count (0 = the cost
 * model's).  Results stay bit-identical for a given choice.  Returns 0. */
int s2h_wgrad_force(int tile, int splits);

/* Deferred gradient sums (round 5, csrc/grad_defer.hip).  No reference counterpart: the reference's
 * parameter gradients come from torch autograd's per-op accumulation (the LayerNorm / Linear bias
 * backward inside nn.LayerNorm / nn.Linear, hieradet.py:98-166, memory_attention.py:58-99,
 * transformer.py:137-311).  Here those column reductions run as per-block partial rows + a fixed-order
 * sum; between s2h_grad_defer(ws, ...) and s2h_grad_defer(NULL, ...) the fixed-order sums whose
 * destinations lie inside [sink, sink + sink_bytes) (the gradient arena) are recorded instead of
 * launched, their partials kept in ws (device memory owned by the caller, 256-B aligned), and
 * s2h_grad_defer_flush adds them all in a few launches on `stream` (64 records per launch, in record
 * order for overlapping destinations).  Nothing may read those destinations before the flush.
 * s2h_grad_defer(NULL, ...) with records pending returns hipErrorNotReady. */
int s2h_grad_defer(void* ws, int64_t ws_bytes, void* sink, int64_t sink_bytes);
int s2h_grad_defer_flush(hipStream_t stream);
/* ends the deferral scope unconditionally, dropping unflushed records (cleanup after a failed flush).
 * Records are taken from one stream per scope (the first record's); s2h_grad_defer_flush on another
 * stream with records pending returns hipErrorInvalidResourceHandle. */
int s2h_grad_defer_reset(void);
/* records waiting for s2h_grad_defer_flush (not a hipError_t) */
int s2h_grad_defer_pending(void);

/* ---------------------------------------------------------------- MX-fp8 (BASELINE config 5)
 * No reference counterpart: the reference trains in fp32 / bf16 autocast only
 * (trainer.py:256-289 under Lightning `precision`); this is the fp8 variant of the projection
 * and FFN GEMMs the north_star asks for (`s2h_gemm` replaces nn.Linear in hieradet.py:56-91,
 * memory_attention.py:58-99, transformer.py:137-311).  OCP MX v1.0 MXFP8-E4M3: 32-element
 * blocks along the reduction dimension, one E8M0 scale each.
 *
 * s2h_mx8_quant: element (r, c) of X (bf16 / fp32) at X[r*ld_row + c*ld_col], r < rows, c < cols,
 * blocks along c.  Q [rows][ldq] u8 e4m3 (ldq >= cols rounded up to 128, ldq % 16 == 0, Q 16-B
 * aligned; columns cols..ldq-1 of the first round-up written as zeros); S [ceil(cols/128)][lds]
 * int32 scale words (lds >= rows): byte b of word (kt, r) = E8M0 scale of block 4kt+b of row r.
 * ld_row == 1 selects the row-walking lane order (a transposed source). */
int s2h_mx8_quant(int rows, int cols, int dt_x, const void* X, int64_t ld_row, int64_t ld_col, uint8_t* Q,
                  int64_t ldq, int32_t* S, int64_t lds, hipStream_t stream);

/* C[M, N] = epilogue(alpha * A B^T) for MX-fp8 A [M, K] (Q lda, scales SA, row stride lsa >= M)
 * and B [N, K] (ldb, SB, lsb >= N) as s2h_mx8_quant writes them; K is the logical depth (both
 * operands zero-padded to a multiple of 128).  Epilogue as s2h_gemm with bias per column:
 * act (aux_mode 1 stores the pre-activation to X, 2 multiplies by act'(X)), dropout, residual R,
 * beta.  C bf16 (dt_c 1) or fp32 (0); R and X are bf16 whatever dt_c is (row strides ldr / ldx in
 * elements); the dropout probability is quantised to 1/65536 as in s2h_gemm. */
int s2h_gemm_mx8(int M, int N, int K, const uint8_t* A, int64_t lda, const int32_t* SA, int64_t lsa,
                 const uint8_t* B, int64_t ldb, const int32_t* SB, int64_t lsb, void* C, int dt_c, int64_t ldc,
                 const float* bias, const void* R, int64_t ldr, void* X, int64_t ldx, int aux_mode, float drop_p,
                 uint64_t seed, uint64_t drop_idx0, float alpha, float beta, int act, hipStream_t stream);

/* MX-fp8 GEMM tiling override for measurements: 0 automatic, 1 64x64, 2 128x64, 3 128x128;
 * bits 8+ measurement-only ablations (1 skip epilogue stores, 2 skip MFMAs, 4 skip operand DMA);
 * returns the previous value. */
int s2h_mx8_config(int cfg);

/* ---------------------------------------------------------------- attention
 * Fused multi-head attention, tensors [B, L, H, D] addressed through
 * (batch, head, row) strides with contiguous D; lse [B, H, Lq] fp32 (natural log).
 * Optional attention-probability dropout p_drop with a counter-based hash keyed by
 * `seed` (regenerated identically in the backward) over the element index
 * idx0 + ((b*H + h)*Lq + q)*Lk + k.  D in {32, 64, 96, 128, 256}
 * for bf16, 32..256 (multiple of 4) for fp32.
 * Replaces F.scaled_dot_product_attention at hieradet.py:70 (windowed / global
 * Hiera attention), transformer.py:243 (two-way decoder attention) and
 * transformer.py:306 (memory-attention RoPE self / cross attention).
 * bf16 with head_dim 256, or 32..128 in steps of 8 (run in a zero-padded 64 / 128 image: Hiera-B+'s
 * 56, Hiera-L's 72), and >= 128 query rows takes the flash path
 * (16x16x32 MFMA, LDS-DMA K/V ring, key range split over workgroups): it wants a
 * device workspace of s2h_attn_fwd_ws_bytes(...) bytes (ws = NULL / too small
 * just disables the key split). */
int64_t s2h_attn_fwd_ws_bytes(int dt, int B, int H, int Lq, int Lk, int D);
/* A/B switch (tests, benchmarks): bit 0 of flash_enable = 0 sends every attention to the
 * generic kernels; bits 8+ (if non-zero) set the workgroup count the flash forward key split
 * aims at (default 256).  Returns the previous setting in the same encoding. */
/* A/B knob: 1 (default) runs bf16 attentions with Lq, Lk <= 64, head dim <= 64 and no dropout (the
 * Hiera windows) on the whole-instance small-window kernels (attention.hip attn_win_*), 0 on the
 * tile kernels.  Returns the previous setting. */
int s2h_attn_win(int on);
int s2h_attn_config(int flash_enable);
/* A/B bits (round 6, default 0) of the non-V-fold flash kernels: 1 the head-dim-256 self-attention dQ
 * kernel with 8 fragment reads ahead, 2 the head-dim <= 128 dQ kernel on a 3-stage ring, 4 the
 * head-dim <= 128 forward on a 3-stage ring, 8 the 32x32 dK / dV kernel on a 3-stage ring, 16 the
 * one-row-per-wave key-split combine (all flash forwards, V-fold included).  Returns the previous bits
 * (mode < 0: query only). */
int s2h_flash_variant2(int mode);
/* A/B knob (round 6): fp32 GEMMs of fewer than 64 tiles of 64 x 64 on 32 x 32 tiles (1, default) or 64 x 64
 * (0).  Returns the previous mode (mode < 0: query only). */
int s2h_gemm_f32_small(int mode);
int s2h_attn_fwd(int dt, int B, int H, int Lq, int Lk, int D,
                 const void* q, int64_t sqb, int64_t sqh, int64_t sql,
                 const void* k, int64_t skb, int64_t skh, int64_t skl,
                 const void* v, int64_t svb, int64_t svh, int64_t svl,
                 void* o, int64_t sob, int64_t soh, int64_t sol,
                 float* lse, float scale, float p_drop, uint64_t seed, uint64_t idx0, uint32_t* keep,
                 void* ws, int64_t ws_bytes, hipStream_t st);
/* Dropout keep bitmap (`keep`, nullable, p_drop > 0 only): the flash forward at head_dim 256
 * also writes each element's keep flag -- bit (k & 31) of word [(b*H + h) * Lq + q] * kw + k/32,
 * kw = 2 * ceil(Lk / 64); s2h_attn_keep_words(...) words -- and the backward reads it instead
 * of re-hashing.  A non-NULL keep on a launch that does not take that path is an error. */
int64_t s2h_attn_keep_words(int B, int H, int Lq, int Lk);
/* Backward of s2h_attn_fwd; di_ws: fp32 workspace [B*H*Lq].  The flash forward's domain takes
 * the flash path (dQ kernel with key-split fp32 partials in
 * `ws` of s2h_attn_bwd_ws_bytes(...) bytes, dK/dV kernel per 128-key block). */
int64_t s2h_attn_bwd_ws_bytes(int dt, int B, int H, int Lq, int Lk, int D);
int s2h_attn_bwd(int dt, int B, int H, int Lq, int Lk, int D,
                 const void* q, int64_t sqb, int64_t sqh, int64_t sql,
                 const void* k, int64_t skb, int64_t skh, int64_t skl,
                 const void* v, int64_t svb, int64_t svh, int64_t svl,
                 const void* o, int64_t sob, int64_t soh, int64_t sol,
                 const void* dout, int64_t sgb, int64_t sgh, int64_t sgl,
                 void* dq, int64_t sdqb, int64_t sdqh, int64_t sdql,
                 void* dk, int64_t sdkb, int64_t sdkh, int64_t sdkl,
                 void* dv, int64_t sdvb, int64_t sdvh, int64_t sdvl,
                 const float* lse, float* di_ws, float scale, float p_drop, uint64_t seed, uint64_t idx0,
                 const uint32_t* keep, void* ws, int64_t ws_bytes, hipStream_t st);
/* Frame-batched flash backward (the flash domain: bf16, head_dim 32..128 / 256, Lq >= 128):
 * nfr frames x bpf batches x H heads of the tracking loop in one launch per kernel -- Q / O / dO /
 * dQ / lse uniform [nfr*bpf] batches, K / V / dK / dV packed per frame (frame f: bpf blocks of fr_lk[f] rows
 * starting at row fr_krow[f]); frame f's dropout indices start at fr_idx0[f] (host arrays of
 * nfr <= 32 entries); keep (nullable) = the frames' forward keep bitmaps, frame f's from word
 * fr_koff[f].  The memory-attention backward of every frame at once
 * (transformer.py:275-311 for frames 1..T-1, memory_attention.py:58-99). */
/* 1 when s2h_flash_bwd_frames takes (dt, Lq, head_dim); 0 = run the frames one by one. */
int s2h_flash_bwd_ok(int dt, int Lq, int D);
int s2h_flash_bwd_frames(int nfr, int bpf, int H, int Lq, int D, const int* fr_lk, const int64_t* fr_krow,
                         const uint64_t* fr_idx0, const void* q, int64_t sqb, int64_t sqh, int64_t sql,
                         const void* k, int64_t skh, int64_t skl, const void* v, int64_t svh, int64_t svl,
                         const void* o, int64_t sob, int64_t soh, int64_t sol, const void* dout, int64_t sgb,
                         int64_t sgh, int64_t sgl, void* dq, int64_t sdqb, int64_t sdqh, int64_t sdql, void* dk,
                         int64_t sdkh, int64_t sdkl, void* dv, int64_t sdvh, int64_t sdvl, const float* lse,
                         float* di_ws, float scale, float p_drop, uint64_t seed, const uint32_t* keep,
                         const int64_t* fr_koff, hipStream_t st);
/* s2h_flash_bwd_frames with the q projection's RoPE epilogue transposed into the dQ store
 * (position_encoding.py:212-239 apply_rotary_enc, transposed; head dim 256; replaces the separate
 * rotation pass over dq of the memory self-attention, transformer.py:296-307): query rows
 * < fr_nrotq[f] of every batch block of frame f are rotated back with table row (row % rope_period)
 * of cos / sin [period, 128] fp32 (fr_nrotq NULL: unrotated); dk is stored unrotated. */
int s2h_flash_bwd_frames_rope(int nfr, int bpf, int H, int Lq, int D, const int* fr_lk, const int64_t* fr_krow,
                              const uint64_t* fr_idx0, const void* q, int64_t sqb, int64_t sqh, int64_t sql,
                              const void* k, int64_t skh, int64_t skl, const void* v, int64_t svh, int64_t svl,
                              const void* o, int64_t sob, int64_t soh, int64_t sol, const void* dout, int64_t sgb,
                              int64_t sgh, int64_t sgl, void* dq, int64_t sdqb, int64_t sdqh, int64_t sdql, void* dk,
                              int64_t sdkh, int64_t sdkl, void* dv, int64_t sdvh, int64_t sdvl, const float* lse,
                              float* di_ws, float scale, float p_drop, uint64_t seed, const uint32_t* keep,
                              const int64_t* fr_koff, const float* rope_cos, const float* rope_sin, int rope_period,
                              const int* fr_nrotq, hipStream_t st);

/* V-fold of the memory-attention cross-attention (RoPEAttention, transformer.py:275-311, with
 * kv_in_dim 64: memory_attention.py:66-81, sam2.1_hiera_t.yaml:49-58).  Its values are a projection
 * of the 64-channel memory bank M, V = M Wv^T + bv, so with D = dropout(softmax(scale q k^T))
 * (the dropped, normalised probabilities) attention(q, k, V) = u' [Wv | bv]^T where
 * u' = [D M | rowsum(D) | 0 x 7] (72 columns).  Single head, q / k head_dim 256, bf16, Lq >= 128.
 * s2h_attn_fwd_vfold: q [B, Lq, 256], k [B, Lk, 256] (RoPE applied), mem [B, Lk, 64] -> u [B, Lq,
 * sul >= 72], lse [B, Lq]; strides (batch, row) in elements, 16-B aligned rows; ws of
 * s2h_attn_fwd_vfold_ws_bytes bytes enables the key split; keep: as s2h_attn_fwd (B, H = 1).
 * Replaces v_proj(memory) + the SDPA of the cross-attention (transformer.py:296-307). */
int64_t s2h_attn_fwd_vfold_ws_bytes(int B, int Lq, int Lk);
int s2h_attn_fwd_vfold(int B, int Lq, int Lk, const void* q, int64_t sqb, int64_t sql, const void* k, int64_t skb,
                       int64_t skl, const void* mem, int64_t smb, int64_t sml, void* u, int64_t sub, int64_t sul,
                       float* lse, float scale, float p_drop, uint64_t seed, uint64_t idx0, uint32_t* keep, void* ws,
                       int64_t ws_bytes, hipStream_t st);
/* Frame-batched backward of s2h_attn_fwd_vfold (layout as s2h_flash_bwd_frames, H = 1): du = the
 * gradient of u' (dO [Wv | bv | 0], 72 columns), dq, dk; no value gradient (the memory bank is
 * detached, sam2model.py:345-358).  di_ws: fp32 [nfr * bpf * Lq]. */
int s2h_flash_bwd_frames_vfold(int nfr, int bpf, int Lq, const int* fr_lk, const int64_t* fr_krow,
                               const uint64_t* fr_idx0, const void* q, int64_t sqb, int64_t sql, const void* k,
                               int64_t skl, const void* mem, int64_t sml, const void* u, int64_t sub, int64_t sul,
                               const void* du, int64_t sgb, int64_t sgl, void* dq, int64_t sdqb, int64_t sdql, void* dk,
                               int64_t sdkl, const float* lse, float* di_ws, float scale, float p_drop, uint64_t seed,
                               const uint32_t* keep, const int64_t* fr_koff, hipStream_t st);
/* The same with the keys' inverse RoPE fused into the dK store (position_encoding.py:212-239
 * apply_rotary_enc with repeat_freqs_k, transposed; replaces the separate rotation pass over dk):
 * key rows < fr_nrot[f] of every batch block of frame f are rotated back with table row
 * key % rope_period of cos / sin [period, 128] fp32 (head dim 256, every column rotated); the
 * remaining rows (object-pointer keys) are stored as computed.  rope_cos == NULL: no rotation. */
int s2h_flash_bwd_frames_vfold_rope(int nfr, int bpf, int Lq, const int* fr_lk, const int64_t* fr_krow,
                                    const uint64_t* fr_idx0, const void* q, int64_t sqb, int64_t sql, const void* k,
                                    int64_t skl, const void* mem, int64_t sml, const void* u, int64_t sub, int64_t sul,
                                    const void* du, int64_t sgb, int64_t sgl, void* dq, int64_t sdqb, int64_t sdql,
                                    void* dk, int64_t sdkl, const float* lse, float* di_ws, float scale, float p_drop,
                                    uint64_t seed, const uint32_t* keep, const int64_t* fr_koff, const float* rope_cos,
                                    const float* rope_sin, int rope_period, const int* fr_nrot, hipStream_t st);
/* + the query projection's inverse RoPE in the dQ store (query rows < fr_nrotq[f], same tables;
 * transformer.py:296 q rotation transposed).  fr_nrot / fr_nrotq each NULL: that gradient unrotated. */
int s2h_flash_bwd_frames_vfold_rope_qk(int nfr, int bpf, int Lq, const int* fr_lk, const int64_t* fr_krow,
                                       const uint64_t* fr_idx0, const void* q, int64_t sqb, int64_t sql, const void* k,
                                       int64_t skl, const void* mem, int64_t sml, const void* u, int64_t sub,
                                       int64_t sul, const void* du, int64_t sgb, int64_t sgl, void* dq, int64_t sdqb,
                                       int64_t sdql, void* dk, int64_t sdkl, const float* lse, float* di_ws,
                                       float scale, float p_drop, uint64_t seed, const uint32_t* keep,
                                       const int64_t* fr_koff, const float* rope_cos, const float* rope_sin,
                                       int rope_period, const int* fr_nrot, const int* fr_nrotq, hipStream_t st);
/* [Wv | bv | 0] as a bf16 [N, ld] matrix (ld >= K + 1) from the bf16 weight [N, K] and the fp32 bias,
 * and its fp32 gradient g [N, ld] scattered back: gwv [N, K] += g[:, :K], gbv [N] += g[:, K]
 * (either nullable).  The value projection's parameters of the folded cross-attention. */
int s2h_vfold_weight(int N, int K, int ld, const void* wv, const float* bv, void* out, hipStream_t st);
int s2h_vfold_grad(int N, int K, int ld, const float* g, float* gwv, float* gbv, hipStream_t st);

/* bf16 Linear whose output is rotated by the axial RoPE in the GEMM epilogue: Y = A W^T + bias
 * (A [M, K], W [N, K] rows K-contiguous), then in every block of L rows the rows r < nrot are
 * rotated in (2i, 2i+1) column pairs for columns c < ncol with table row r % period and column
 * (c % dh) / 2 (cosv / sinv [period, dh / 2] fp32, as s2h_rope).  Replaces q_proj / k_proj +
 * apply_rotary_enc (transformer.py:275-311, position_encoding.py:212-239) and the fused
 * q / k / v projection of the memory self-attention with q and k rotated (ncol = 2 x 256). */
int s2h_linear_rope(int M, int N, int K, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                    void* Y, int64_t ldy, const float* cosv, const float* sinv, int L, int nrot, int period, int ncol,
                    int dh, hipStream_t stream);
/* Linear + dropout + residual + LayerNorm in one launch (bf16): C = R + dropout(A W^T + bias)
 * (the residual stream x'), Y = LN(C) * gamma + beta, mean / rstd per row -- a projection and the
 * residual add + LayerNorm that reads it (memory_attention.py:60-98: out_proj -> norm2, the
 * cross-attention output -> norm3, linear2 -> the next layer's norm1; nn.LayerNorm).  N = 128 or 256
 * (one workgroup per 64 full rows); A [M, K] (lda), W [N, K] (ldw), R / C / Y with row strides;
 * 16-B aligned rows.  R may be NULL (no residual); dropout index = drop_idx0 + row * N + col. */
int s2h_linear_add_ln(int M, int N, int K, const void* A, int64_t lda, const void* W, int64_t ldw,
                      const float* bias, const void* R, int64_t ldr, float drop_p, uint64_t seed,
                      uint64_t drop_idx0, void* C, int64_t ldc, const float* gamma, const float* beta, float eps,
                      void* Y, int64_t ldy, float* mean, float* rstd, hipStream_t st);
/* Backward twin: input gradient of a Linear whose input is a LayerNorm output read by nothing else,
 * with that LayerNorm's backward in the GEMM epilogue (bf16): dy = alpha * G W (G [M, K] the Linear's
 * output gradient, W [K, N] its weight), dx = LN'(dy; X, gamma, mean, rstd) + dres (C [M, N]),
 * dgamma / dbeta += (both or neither; `part` = s2h_linear_dgrad_ln_bwd_ws_bytes(M, N) bytes of
 * per-tile partial rows).  Replaces linear dgrad + s2h_layernorm_bwd for memory_attention.py:60-98
 * norm1 -> q/k/v, norm2 -> cross-attention q, norm3 -> linear1 (torch autograd of nn.Linear +
 * nn.LayerNorm).  N = 128 or 256; 16-B aligned rows; dres may be NULL. */
/* Memory-attention FFN backward, input-gradient side, one launch (bf16; memory_attention.py:97,
 * replacing torch autograd's linear2 input gradient -> ReLU/dropout backward -> linear1 input gradient):
 *   dh [R, H] = alpha * (dy [R, 256] w2 [256, H]) * [hid > 0]     (alpha = 1 / keep)
 *   dx [R, 256] = dh w1 [H, 256]
 * hid = linear2's saved input (ReLU -> dropout output).  R a multiple of 64, H of 128; 16-B aligned
 * bases, row strides multiples of 8 elements. */
int s2h_ffn_bwd_dgrad(int R, int H, const void* dy, int64_t lddy, const void* w2, const void* w1, const void* hid,
                      int64_t ldh, float alpha, void* dh, int64_t lddh, void* dx, int64_t lddx, hipStream_t st);
/* Memory-attention FFN forward, one launch (bf16; memory_attention.py:97, replacing linear1 + ReLU +
 * dropout and linear2 + dropout as two GEMM launches):
 *   hid [R, H] = drop1(relu(x [R, 256] w1 [H, 256]^T + b1))      (saved for the backward)
 *   y [R, 256] = drop2(hid w2 [256, H]^T + b2)
 * b1 / b2 fp32; dropout p with the GEMM epilogue's counter hash (seed1, element idx1 + row * H + h;
 * seed2, idx2 + row * 256 + n), each seed folded with the bound RNG offset.  R a multiple of 64, H 1024
 * or 2048; 16-B aligned bases, row strides multiples of 8 elements. */
int s2h_ffn_fwd(int R, int H, const void* x, int64_t ldx, const void* w1, const float* b1, const void* w2,
                const float* b2, float p, uint64_t seed1, uint64_t idx1, uint64_t seed2, uint64_t idx2, void* hid,
                int64_t ldh, void* y, int64_t ldy, hipStream_t st);
/* Two-way transformer token side, forward (bf16; sam/transformer.py:112-197, replacing per block ~17
 * of ~17 launches (13 objects x 8 tokens) to five).  R = objects x T rows (T <= 16
 * tokens per object, an object never split), width 256, self-attention 8 heads of 32, cross-attention
 * width 128, MLP 256 -> 2048 -> 256 ReLU; weights [N, K] bf16 row-major, biases / LayerNorm fp32.  Every
 * intermediate is written where the frame tape stores the corresponding op's output (lse [objects, 8,
 * T] natural log; mean / rstd per row).
 * s2h_dec_self (transformer.py:163-170): qa = x + pe (skip == 0, else unused), q / k from (skip ? x : qa),
 *   v from x, os = self-attention, y1 = os Wo^T + bo (+ x unless skip), x1 = norm1(y1), qt = x1 + pe,
 *   qq = qt Wqc^T + bqc (the token -> image query). */
int s2h_dec_self(int R, int T, int skip, float scale, const void* x, const void* pe, const void* wq, const float* bq,
                 const void* wk, const float* bk, const void* wv, const float* bv, const void* wo, const float* bo,
                 const float* g1, const float* b1, float eps1, const void* wqc, const float* bqc, void* qa, void* qs,
                 void* ks, void* vs, void* os, float* lse, void* y1, void* x1, float* mean1, float* rstd1, void* qt,
                 void* qq, hipStream_t st);
/* A/B knob (round 6): 1 (default) the s2h_dec_* kernels issue each projection's weight fragments a phase
 * ahead (s2h_dec_self: the q / k / v weights together, the out- and q-projection weights under the
 * attention and norm1; the others: under their row loads and LayerNorms), 0 each projection loads its own
 * before its MFMAs; the same sums either way.  Returns the previous setting
 * (mode < 0: query only). */
int s2h_dec_sched(int mode);
/* The second half's token side around the MLP (whose two GEMMs stay s2h_gemm launches; transformer.py:170-173):
 * s2h_dec_post_a: y2 = ot Wo^T + bo + x1, x2 = norm2(y2);
 * s2h_dec_post_b: x3 = norm3(y3) (y3 = MLP output + x2), q2 = x3 + pe, kio = q2 Wki^T + bki,
 *   vio = x3 Wvi^T + bvi (the image -> token keys / values); final_q: qfa = x3 + pe, qqf = qfa Wqf^T + bqf
 *   (TwoWayTransformer's final token -> image query, :194-196). */
int s2h_dec_post_a(int R, int T, const void* ot, const void* x1, const void* wo, const float* bo, const float* g2,
                   const float* b2n, float eps2, void* y2, void* x2, float* mean2, float* rstd2, hipStream_t st);
int s2h_dec_post_b(int R, int T, int final_q, const void* y3, const void* pe, const float* g3, const float* b3n,
                   float eps3, const void* wki, const float* bki, const void* wvi, const float* bvi, const void* wqf,
                   const float* bqf, void* x3, float* mean3, float* rstd3, void* q2, void* kio, void* vio, void* qfa,
                   void* qqf, hipStream_t st);
/* s2h_dec_final (transformer.py:196-197): y = of Wo^T + bo + x3, hs = norm(y). */
int s2h_dec_final(int R, int T, const void* of, const void* x3, const void* wo, const float* bo, const float* g,
                  const float* bn, float eps, void* y, void* hs, float* mean, float* rstd, hipStream_t st);
int64_t s2h_linear_dgrad_ln_bwd_ws_bytes(int M, int N);
int s2h_linear_dgrad_ln_bwd(int M, int N, int K, const void* G, int64_t ldg, const void* W, int64_t ldw, float alpha,
                            const void* X, int64_t ldx, const float* gamma, const float* mean, const float* rstd,
                            const void* dres, int64_t ldr, void* dx, int64_t lddx, float* part, float* dgamma,
                            float* dbeta, hipStream_t st);
/* dgamma += sum_b part[b][0:C], dbeta += sum_b part[b][C:2C] over nb partial rows of 2C floats. */
int s2h_ln_wgrad_finalize(int nb, int C, const float* part, float* dgamma, float* dbeta, hipStream_t st);

/* Per-object MLP heads under no_grad in ONE launch (bf16): for each of nheads (<= 8) heads, rows
 * x[h] [M, dims[4h]] (row stride ldx[h]) through nl[h] (<= 3) Linear layers w[3h + l]
 * [dims[4h+l+1], dims[4h+l]] (+ fp32 bias b[3h + l] or NULL), ReLU between layers, act_last[h]
 * (S2HAct) after the last, into y[h] [M, dims[4h + nl]] (row stride ldy[h]); widths <= 256 (hidden
 * ones multiples of 8), 16-B aligned rows.  Bit-identical to the per-layer GEMMs.  Replaces the
 * object-score head (mask_decoder.py:234-238) and the object-pointer projection (sam2_base.py:296-305
 * obj_ptr_proj): 6 launches of 13 rows per frame -> 1.  Argument arrays are host memory. */
int s2h_mlp_heads(int nheads, int M, const void* const* x, const int64_t* ldx, const void* const* w,
                  const float* const* b, const int* dims, const int* nl, const int* act_last, void* const* y,
                  const int64_t* ldy, void* const* hid, void* const* pre, hipStream_t st);
/* (hid[2h + l], optional: layer l's ReLU output [M, dims[4h+l+1]] for l < nl - 1; pre[h], optional:
 * the last layer's pre-activation -- saved for the backward of trained heads: the mask decoder's
 * hypernetwork MLP and IoU head, mask_decoder.py:227-233, in the frame-batched tape) */

/* ---------------------------------------------------------------- normalisation
 * Row LayerNorm over C (<= 1280) with an optional fused pre-add:
 * xsum = x + badd (badd broadcast over rows when b_bcast), y = LN(xsum) * gamma + beta;
 * saves per-row mean / rstd (fp32).  Replaces nn.LayerNorm (hieradet.py:134-166,
 * memory_attention.py:43-45,115, transformer.py:63,137-149) and LayerNorm2d
 * (sam2_utils.py:141-151, NHWC rows) and the residual adds feeding them. */
int s2h_layernorm_fwd(int dt, int rows, int C, const void* x, int64_t ldx, const void* badd, int64_t ldb,
                      int b_bcast, void* xsum, const float* gamma, const float* beta, float eps, void* y,
                      int64_t ldy, float* mean, float* rstd, hipStream_t st);
/* bf16 LayerNorm of contiguous rows that also stores ype = y + pe[row % pe_rows] (the two-way
 * transformer's keys + key_pe after norm4, transformer.py:182-185 feeding the next block's
 * k = keys + key_pe, transformer.py:170 / :102): y bit-identical to s2h_layernorm_fwd, ype to the
 * broadcast add it replaces.  16-B aligned rows, C / 8 <= 64. */
int s2h_layernorm_fwd_pe(int dt, int rows, int C, const void* x, const float* gamma, const float* beta, float eps,
                         void* y, float* mean, float* rstd, const void* pe, int pe_rows, void* ype, hipStream_t st);
/* dx = LN'(dy) (+= when dx_accum, or + dres: the residual-stream gradient of the fused
 * pre-add, so the caller needs no copy), dgamma += , dbeta += (fp32, both or neither).
 * The weight gradients go through per-block partials in `ws`
 * (s2h_layernorm_bwd_ws_bytes(dt, rows, C) bytes; may be NULL when dgamma is NULL). */
int64_t s2h_layernorm_bwd_ws_bytes(int dt, int rows, int C);
int s2h_layernorm_bwd(int dt, int rows, int C, const void* x, int64_t ldx, const void* dy, int64_t lddy,
                      const float* gamma, const float* mean, const float* rstd, void* dx, int64_t lddx,
                      int dx_accum, const void* dres, int64_t ldres, float* dgamma, float* dbeta, void* ws,
                      hipStream_t st);

/* ---------------------------------------------------------------- elementwise / layout
 * out = alpha*a + beta*b (residual adds, sam2_base.py:680-684 no_mem_embed,
 * memory_attention.py:140-141 curr + 0.1*pos). */
int s2h_add(int dt, int64_t n, const void* a, const void* b, float alpha, float beta, void* out, hipStream_t st);
/* out[o, i] = alpha*a[o, i] + beta*b[i % b_period] (bias / embedding broadcast:
 * mask_decoder.py:201-209 dense prompt add, sam2_base.py:761-767 no_obj_embed_spatial). */
int s2h_add_bcast(int dt, int64_t outer, int64_t inner, const void* a, float alpha, const void* b,
                  int64_t b_period, float beta, void* out, hipStream_t st);
/* y = act(scale*x + shift) (GELU / ReLU / sigmoid; sam2_base.py:742-747 mask_for_mem). */
int s2h_act_fwd(int dt, int64_t n, const void* x, int act, float scale, float shift, void* y, hipStream_t st);
/* dx (=, or += when accum) = dy * act'(x). */
int s2h_act_bwd(int dt, int64_t n, const void* x, const void* dy, int act, void* dx, int accum, hipStream_t st);
/* dtype conversion (fp32 <-> bf16; sam2_base.py:391-399 `.float()` of the logits). */
int s2h_cast(int dt_in, int dt_out, int64_t n, const void* x, void* y, hipStream_t st);
/* out = a + dropout(b) (b may be NULL: out = dropout(a)), element index idx0 + i; nn.Dropout at
 * memory_attention.py:40-48 and the post-attention / FFN dropouts. */
int s2h_dropout(int dt, int64_t n, const void* a, const void* b, float p, uint64_t seed, uint64_t idx0, void* out,
                hipStream_t st);
/* dx = act'(x_pre) * keep(i) / (1 - p) * dy in one pass: the backward of a Linear epilogue's
 * act -> dropout (memory_attention.py:95-98); x_pre NULL = no activation. */
int s2h_act_dropout_bwd(int dt, int64_t n, const void* x_pre, const void* dy, int act, float p, uint64_t seed,
                        uint64_t idx0, void* dx, hipStream_t st);
/* dx = scale * [y > 0] * dy: the backward of ReLU (-> dropout, scale = 1/(1-p)) from the layer's
 * output y, which is positive exactly where the pre-activation was and the element was kept
 * (memory_attention.py:95-98 linear1 + ReLU + dropout; no pre-activation stored, no re-hash). */
int s2h_relu_mask_bwd(int dt, int64_t n, const void* y, const void* dy, float scale, void* dx, hipStream_t st);
/* Axial rotary embedding of the first `nrot` rows of each batch (cos/sin tables
 * [period, D/2], row r uses entry r % period; inverse = 1 applies the transpose
 * rotation for the backward).  Replaces apply_rotary_enc (position_encoding.py:212-239)
 * with compute_axial_cis tables (:192-201) and the key-repeat at transformer.py:291-299. */
int s2h_rope(int dt, int64_t nb, int nrot, int D, const void* x, int64_t sxb, int64_t sxl, void* y,
             int64_t syb, int64_t syl, const float* cosv, const float* sinv, int period, int inverse,
             hipStream_t st);
/* 2x2/2 max pooling, NHWC with pixel stride ldx (do_pool, hieradet.py:25-36). */
int s2h_maxpool2_fwd(int dt, int B, int H, int W, int C, const void* x, int64_t ldx, void* y, hipStream_t st);
int s2h_maxpool2_bwd(int dt, int B, int H, int W, int C, const void* x, int64_t ldx, const void* dy,
                     void* dx, int64_t lddx, hipStream_t st);
/* Up to 16 strided 2-D copies in one launch (replaces torch.cat / copy_ of the memory bank
 * assembly, reference sam2_base.py:649-676, and the tracking loop's per-frame gradient packing):
 * segment s copies rows[s] rows of row_bytes[s] bytes from src[s] (pitch src_ld[s] bytes) to dst[s]
 * (pitch dst_ld[s]; destination rows must not overlap, a source pitch of 0 broadcasts).  Host arrays
 * of n entries; bases, pitches and row lengths 4-B aligned (16-B aligned segments move in 16-B
 * pieces), else hipErrorInvalidValue. */
int s2h_copy2d_batch(int n, const void* const* src, void* const* dst, const int64_t* rows, const int64_t* row_bytes,
                     const int64_t* src_ld, const int64_t* dst_ld, hipStream_t st);
/* window_partition (dir 0) / window_unpartition (dir 1) with zero padding
 * (backbones/utils.py:16-60); accum adds into dst. */
int s2h_window(int dt, int B, int H, int W, int C, int ws, const void* src, void* dst, int dir, int accum,
               hipStream_t st);
/* window_partition of a per-token projection's output with the padded positions set to padrow
 * (fp32 [C], rounded to dt): with padrow = the projection's bias this equals the projection of the
 * zero-padded partition (hieradet.py:146 pads before attn.qkv), so the projection runs over the real
 * tokens only.  C a multiple of 16 B, 16-B aligned tensors. */
int s2h_window_pad(int dt, int B, int H, int W, int C, int ws, const void* src, const float* padrow, void* dst,
                   hipStream_t st);
/* Its bias gradient: out[c] += sum of win[row][c] over the padded rows of the windowed tensor
 * (fixed-order partial sums). */
int s2h_window_pad_colsum(int dt, int B, int H, int W, int C, int ws, const void* win, float* out, hipStream_t st);
/* The same over rows that are already compact: src [B * P][C] bf16 holds only the padded rows, in that
 * enumeration order (per image the rows y >= H, then x >= W); same chunks and fixed-order finish, so
 * every column's sum has the bits s2h_window_pad_colsum gives for the partitioned tensor. */
int s2h_pad_rows_colsum(int B, int P, int C, const void* src, float* out, hipStream_t st);
/* Padded-window attention straight from the image layout (Hiera's windows that need padding,
 * hieradet.py:146; bf16, head dim hd 32..128, ws * ws in [128, 512]).  s2h_window_map builds the row
 * map of a geometry on the host: n = s2h_window_map_len ints, [row: nW x L][padidx: nW x L][sets: nW]
 * (L = ws * ws, nW windows per image; row = token index y * W + x or -1 for padding; padidx = the
 * padded position's row in s2h_pad_rows_colsum's order or -1; sets = bit s set when positions
 * 16 s .. 16 s + 15 hold a token), every entry range-checked.  The kernels take a device copy.
 * s2h_flash_win_ok: 1 when the mode applies to (dt, batch, geometry) -- it needs enough batch-heads
 * that the partitioned launches would not split their key range; 0 = partition and use s2h_attn_*.
 * Forward: qkv [B, H, W, 3 d] (d = NH * hd), padrow [3 d] bf16 (the projection's bias, as
 * s2h_window_pad rounds it) -> o [B, H, W, d], lse [B * nW * NH][L] (+inf at padded positions).
 * Backward: dout [B, H, W, d], zrow >= hd zeros -> dqkv [B, H, W, 3 d] (every real token's dq | dk | dv),
 * dpad [B * P][2 d] (dk | dv of the padded keys); di [B * nW * NH][L] scratch.  Results equal the
 * partitioned path's bit for bit. */
int64_t s2h_window_map_len(int H, int W, int ws);
int s2h_window_map(int H, int W, int ws, int* out, int64_t n);
int s2h_flash_win_ok(int dt, int B, int H, int W, int ws, int NH, int hd);
int s2h_flash_win_fwd(int B, int H, int W, int ws, int NH, int hd, const void* qkv, const void* padrow, const int* map,
                      void* o, float* lse, float scale, hipStream_t st);
int s2h_flash_win_bwd(int B, int H, int W, int ws, int NH, int hd, const void* qkv, const void* padrow,
                      const void* zrow, const int* map, const void* o, const void* dout, void* dqkv, void* dpad,
                      const float* lse, float* di, float scale, hipStream_t st);
/* FPN top-down: out = lat + nearest_up2(prev) (image_encoder.py:102-134). */
int s2h_up2_add(int dt, int B, int H, int W, int C, const void* lat, const void* prev, void* out, hipStream_t st);
/* Backward of the nearest 2x upsample: dprev (+)= 2x2 sum of dout. */
int s2h_pool2_sum(int dt, int B, int Ho, int Wo, int C, const void* dout, void* dprev, int accum, hipStream_t st);
/* Bilinear resize, align_corners=False, fp32 [N, hi, wi] -> [N, ho, wo]
 * (F.interpolate at sam2_base.py:393-399, low-res -> high-res mask logits). */
int s2h_bilinear_fwd(int N, int hi, int wi, int ho, int wo, const float* x, float* y, hipStream_t st);
int s2h_bilinear_bwd(int N, int hi, int wi, int ho, int wo, const float* dy, float* dx, hipStream_t st);
/* out[c] (=, or += when accum) = sum_r x[r, c] (bias gradients). */
int s2h_colsum(int dt, int64_t rows, int cols, const void* x, int64_t ld, float* out, int accum, hipStream_t st);
/* Segmented column sums, one launch: out[dsts[s], c] += sum_{r < rows} x[offs[s] + r, c] for s < nseg
 * (<= 64; cols a multiple of the 16-B vector, <= 256 vectors).  The memory positions' temporal-code
 * gradient (sam2_base.py:605-611: maskmem_tpos_enc added per memory slot), all slots of all frames. */
int s2h_colsum_seg(int dt, int nseg, int64_t rows, int cols, const void* x, int64_t ld, const int64_t* offs,
                   const int* dsts, float* out, hipStream_t st);
/* Memory positions, one launch: out[j L + l, :] = pos[l, :] + tpos[idx[j], :] for j < n (<= 16)
 * (sam2_base.py:605-611: the memory encoder position + maskmem_tpos_enc[t] per memory slot). */
int s2h_memory_pos(int dt, int n, int L, int Dm, const void* pos, const void* tpos, const int* idx, void* out,
                   hipStream_t st);
/* out[i] (=/+=) sum_o x[o, i] (gradient of a per-object broadcast of shared
 * features: sam2model.py:307-311, mask_decoder.py:201,209 repeat_interleave). */
int s2h_sum_outer(int dt, int O, int64_t inner, const void* x, void* out, int accum, hipStream_t st);
/* out[f][:] (+)= sum over o < O of x[f][o][:] for F frames in one launch (x [F, O, inner], out [F, inner];
 * the frame-batched backward of a broadcast over objects, tracking.py / mask_decoder.py); each element
 * summed in o order (the values of F s2h_sum_outer launches). */
int s2h_sum_outer_batched(int dt, int F, int O, int64_t inner, const void* x, void* out, int accum,
                          hipStream_t st);
/* NHWC im2col in PyTorch weight order (c, ky, kx) for the strided convolutions
 * (PatchEmbed utils.py:85; MaskDownSampler memory_encoder.py:43): rows of ldcol >= C*kh*kw elements,
 * the columns past C*kh*kw written as zeros. */
int s2h_im2col(int dt, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int Ho, int Wo,
               int64_t ldcol, const void* x, void* col, hipStream_t st);
/* Mask down-sampler stage, fused 3x3/2 pad-1 conv + LayerNorm2d(cout) + GELU, NHWC
 * (memory_encoder.py:17-55 MaskDownSampler.encoder[3i..3i+2] with the SAM2.1 config
 * kernel_size 3, stride 2, padding 1).  Supported (cin, cout): (1, 4), (4, 16), (16, 64).
 * x_logit: x is the fp32 high-res mask logits [O, H, W] and the stage applies
 * sigmoid(x) * scale + shift first (sam2_base.py:742-747).  Weights fp32 [cout, cin, 3, 3].
 * y [O, ceil(H/2), ceil(W/2), cout]. */
int s2h_mask_down_stage(int dt, int O, int H, int W, int cin, int cout, const void* x, int x_logit, float scale,
                        float shift, const float* w, const float* bias, const float* gamma, const float* beta,
                        float eps, void* y, hipStream_t st);
/* Depthwise KxK conv, NHWC, fp32 weights [C, K, K] (CXBlock dwconv, memory_encoder.py:84). */
int s2h_dwconv(int dt, int B, int H, int W, int C, int K, int pad, const void* x, const float* w,
               const float* bias, void* y, hipStream_t st);
/* ConvTranspose2d k=2 s=2 as GEMM + scatter (dir 0: out = scatter(Y) + bias (+ add));
 * dir 1 gathers the output gradient into GEMM layout (mask_decoder.py:66-75). */
int s2h_convt2(int dt, int B, int H, int W, int Co, const void* Y, const float* bias, const void* add,
               void* out, int dir, hipStream_t st);
/* The forward scatter vectorised with the bias and the residual add fused (round 5; mask_decoder.py:105-107
 * dc1(x) + feat_s1, dc2(x) + feat_s0): out[b, 2y+dy, 2x+dx, co] = Y[(b,y,x)][co*4 + dy*2 + dx] + bias[co]
 * (+ add[b or 0 when add_bcast, 2y+dy, 2x+dx, co]), rounded after the bias and after the add as the
 * two launches it replaces.  Co % (16 B / element) == 0, 16-B aligned buffers. */
int s2h_convt2_store(int dt, int B, int H, int W, int Co, const void* Y, const float* bias, const void* add,
                     int add_bcast, void* out, hipStream_t st);
/* The mask decoder's last upscaling step and mask head in one pass (mask_decoder.py:105-113, bf16,
 * Co = 32): pre = the s2h_convt2_store values, post = gelu(pre) (as s2h_act_fwd rounds it), masks[b][p] =
 * sum_c hyper[b][c] post[b][p][c] (fp32 sum, bf16 store); pre / post [B, 2H, 2W, 32], masks [B, 2H * 2W]. */
int s2h_convt2_tail(int dt, int B, int H, int W, int Co, const void* Y, const float* bias, const void* add,
                    int add_bcast, const void* hyper, void* pre, void* post, void* masks, hipStream_t st);
/* s2h_convt2_tail for all K (= 4) mask tokens of the three-mask heads (inference; mask_decoder.py:227-234):
 * hyper [B, K, 32], masks [B, K, 2H * 2W]; the activation of a pixel is computed once and feeds the K
 * products, each summed in s2h_convt2_tail's order (masks[:, 0] equals its output bit for bit).
 * pre / post may be NULL (forward only). */
int s2h_convt2_tail_k(int dt, int B, int H, int W, int Co, int K, const void* Y, const float* bias, const void* add,
                      int add_bcast, const void* hyper, void* pre, void* post, void* masks, hipStream_t st);
/* Stability counts of mask logits (mask_decoder.py:247-257): counts[2b] = #{p: m[b][p] > delta},
 * counts[2b + 1] = #{p: m[b][p] > -delta} over p < P of row b (row stride ld elements), compared on the
 * stored value widened to fp32; integer sums in a fixed order.  bf16 or fp32. */
int s2h_stability_counts(int dt, int B, int64_t P, const void* masks, int64_t ld, float delta, int* counts,
                         hipStream_t st);
/* Per-object output selection of the three-mask heads (mask_decoder.py:145-166, 259-295 and
 * sam2_base.py:380-420).  masks [B, K, P] (dt), iou [B, K] fp32, score [B] fp32, tok: the K mask tokens
 * of object b at tok + b * ld_tok, each [C] (dt).  best = 1 + first argmax(iou[b][1:K]).
 * mode 0 (multimask): idx = best; mode 1 (dynamic single): idx = 0 when
 * (counts[2b+1] > 0 ? counts[2b] / counts[2b+1] : 1) >= thresh in fp32, else best.
 * Writes idx [B] int32, low [B, P] fp32 = masks[b][idx] where score[b] > 0 else fill, iou_out [B] =
 * iou[b][idx], tok_out [B, C] = token idx when mode 0 and tok_follow, else token 0, and, when not NULL,
 * multi_low [B, K-1, P] fp32 = the gated candidates 1..K-1. */
int s2h_multimask_select(int dt, int B, int K, int64_t P, int C, const void* masks, const float* iou,
                         const int* counts, const float* score, const void* tok, int64_t ld_tok, int mode,
                         int tok_follow, float thresh, float fill, int* idx, float* low, float* iou_out,
                         void* tok_out, float* multi_low, hipStream_t st);
/* 8-connected components of N independent H x W images (upstream sam2/utils/misc.py
 * get_connected_components).  Foreground is scores > 0 when `positive`, scores <= 0 otherwise.
 * labels[p] = 0 off the foreground, else 1 + the smallest row-major index (within its image) of a pixel of
 * p's component; areas[p] = the pixel count of p's component, 0 off the foreground.  Both int32 [N, H, W].
 * A pure function of the input (integer atomics with a unique fixed point, no float atomics), no host
 * round trip, every device loop bounded by 2 H W + 2 steps.  H, W >= 1, H * W <= 2^24,
 * N * H * W < 2^31 - 256. */
int s2h_cc_label(int N, int H, int W, const float* scores, int positive, int* labels, int* areas,
                 hipStream_t st);
/* upstream fill_holes_in_mask_scores on fp32 scores [N, H, W]: first the background components
 * (scores <= 0) of area <= max_area become 0.1f, then, on that result, the foreground components (> 0) of
 * area <= max_area become -0.1f; every other element is copied bit for bit.  work: 2 N H W int32 of
 * scratch; out must not alias scores; max_area >= 1; sizes as for s2h_cc_label. */
int s2h_fill_holes(int N, int H, int W, const float* scores, int max_area, float* out, int* work,
                   hipStream_t st);
/* s2h_cc_label on byte masks [N, H, W]: foreground is mask != 0 when `positive`, mask == 0 otherwise; the same
 * kernels, so labels and areas are those of s2h_cc_label on the corresponding 0 / 1 scores. */
int s2h_cc_label_u8(int N, int H, int W, const uint8_t* mask, int positive, int* labels, int* areas,
                    hipStream_t st);
/* ---- prompts from ground truth (reference sam2_video/eval/inference.py:275-326 get_each_obj, eval/utils.py:95-153
 * mask_to_masks / mask_to_points; csrc/gtprompt.hip).  Common to the five entries below: pure functions of their
 * inputs, integer arithmetic and integer atomics only, every device loop bounded independently of the data, no
 * host round trip; H, W >= 1, H * W <= 2^24, N * H * W < 2^31 - 256 (A in place of N for s2h_rle_decode).
 *
 * COCO RLE -> byte masks (pycocotools mask.decode).  run_end[run_off[a] .. run_off[a + 1]) = the cumulative sums
 * of annotation a's counts: ascending, the last one H W; positions are column-major.  mask [A, H, W] uint8,
 * row-major: pixel (y, x) = k & 1 with k the index of the first run_end > x H + y within the annotation (the
 * number of its runs when there is none).  A zero-length first run (the mask starts set) and a single run (an
 * empty mask) are valid; run_off [A + 1] ascending from 0. */
int s2h_rle_decode(int A, int H, int W, const int* run_off, const int* run_end, uint8_t* mask, hipStream_t st);
/* Offline scoring from the runs (reference sam2_video/eval/eval.py:88-103; csrc/pair_counts.h): group g is one
 * (image, category) pair of H x W images; its predicted annotations are [dt_grp_off[g], dt_grp_off[g + 1]) of
 * dt_run_off / dt_run_end, its ground-truth ones [gt_grp_off[g], gt_grp_off[g + 1]) of gt_run_off / gt_run_end
 * (both in the s2h_rle_decode layout; *_grp_off [G + 1] ascending from 0).  counts[4 g ..] = |p & g|, |p | g|,
 * |p|, |g| as uint64 (zeroed by the call), p and g the OR of the side's annotations; an empty side is an empty
 * mask.  No dense mask is written anywhere; both sides are column-major positions, nothing is transposed.
 * Integer arithmetic and integer atomics only; at most 4096 annotations per group and side are read.  Limits of
 * s2h_rle_decode with G in place of A. */
int s2h_rle_pair_counts(int G, int H, int W, const int* dt_grp_off, const int* dt_run_off, const int* dt_run_end,
                        const int* gt_grp_off, const int* gt_run_off, const int* gt_run_end, uint64_t* counts,
                        hipStream_t st);
/* Rectangular dilation (op 0) or erosion (op 1) of byte masks [N, H, W] (nonzero = set; out is 0 / 1):
 * out(y, x) = OR resp. AND of in(y + dy, x + dx) over dy in [y_lo, y_hi], dx in [x_lo, x_hi], restricted to the
 * positions inside the image -- outside pixels are ignored by both, cv2's default morphology border.
 * -32 <= lo <= 0 <= hi <= 32.  Two separable passes; work: N H W bytes of scratch; in, out and work are three
 * different buffers. */
int s2h_morph_rect(int N, int H, int W, const uint8_t* in, int op, int y_lo, int y_hi, int x_lo, int x_hi,
                   uint8_t* out, uint8_t* work, hipStream_t st);
/* The components of area >= min_area of images labelled by s2h_cc_label(_u8) (labels, areas as it writes them),
 * per image in ascending order of root index = raster order of the first pixel (cv2.connectedComponentsWithStats'
 * order), the images back to back.  grid: [H, W] uint8 or NULL; a pixel of a component is "selected" when
 * grid is NULL or nonzero there.  stats [capacity, 9] int64 per kept component: root label, area, xmin, ymin,
 * xmax, ymax (inclusive, of all its pixels), n_sel, sum x and sum y over its selected pixels.
 * hdr [2 N + 2] int32: count and offset per image, then the total, then a status word: 1 when an image has more
 * than 255 kept components (the index image then saturates at 255 there and must not be used), else 0.  When
 * total > capacity only the first `capacity` rows are written (nothing past the end); the header is complete
 * either way.  index [N, H, W] uint8: 0 = not in a kept component, i = the i-th kept component of its image.
 * work: N H W + N ceil(H W / 256) int32 of scratch.  Additionally N ceil(H W / 256) < 2^31. */
int s2h_cc_components(int N, int H, int W, const int* labels, const int* areas, int min_area, const uint8_t* grid,
                      int capacity, int* hdr, int64_t* stats, uint8_t* index, int* work, hipStream_t st);
/* The q_rank[q]-th pixel, in row-major order, of image q_img[q] among the pixels with
 * (labels == q_label[q]) != (q_neg[q] != 0) that also lie on the grid ([H, W] uint8, NULL = every pixel):
 * np.argwhere(mask & GRID)[rank] of eval/utils.py mask_to_points, for the component (q_neg 0) or its
 * complement (q_neg 1).  xy [Q, 2] int32 = (x, y), (-1, -1) when the rank is negative or not below the count;
 * count [Q] int32 = the number of such pixels (0 for an image index outside [0, N)).
 * work: Q ceil(H W / 4096) int32 of scratch, and Q ceil(H W / 4096) < 2^31. */
int s2h_mask_rank_select(int Q, const int* q_img, const int* q_label, const int* q_neg, const int* q_rank, int N,
                         int H, int W, const int* labels, const uint8_t* grid, int* xy, int* count, int* work,
                         hipStream_t st);
/* ---- correction clicks (reference sam2_video/model/modeling/sam2_utils.py:202-323 sample_random_points_from_errors
 * and sample_one_point_from_error_center; csrc/clicks.hip).  Common to the three entries below: pure functions of
 * their inputs, integer arithmetic only, no atomics, every device loop bounded independently of the data, no host
 * round trip; 1 <= H, W <= 4092, H * W <= 2^24, N * H * W < 2^31 - 256 (B in place of N for the clicks).
 *
 * The exact squared Euclidean distance transform of byte masks [N, H, W] (nonzero = set) with the ring of pixels
 * just outside the image counted as background: dist2(y, x) = 0 where the mask is clear, else the minimum of
 * (y - y')^2 + (x - x')^2 over the (y', x') in [-1, H] x [-1, W] that lie outside the image or where the mask is
 * clear -- the square of cv2.distanceTransform(np.pad(mask, 1), cv2.DIST_L2, 0)[1:-1, 1:-1].  dist2 int32
 * [N, H, W].  work: 2 N H W bytes of scratch. */
int s2h_edt_sq(int N, int H, int W, const uint8_t* mask, int* dist2, void* work, hipStream_t st);
/* The click at the centre of the larger error region, per object b of B: FN = gt & ~pred, FP = ~gt & pred (gt,
 * pred uint8 [B, H, W], nonzero = set; pred NULL = the empty prediction); (dn, in) = the maximum of the distance
 * transform above of FN and the smallest row-major index that reaches it, (dp, ip) the same for FP; label 1 and
 * index in when dn > dp, else label 0 and index ip.  points [B, 2] fp32 = (index % W, index / W); labels [B]
 * int32; dmax [B, 2] int32 = (dn, dp).  Both regions empty: point (0, 0), label 0.  The distances are never
 * written; the argmax is a maximum over the key (D2 << 32) | (0xFFFFFFFF - index), per workgroup and then over
 * the workgroups' partials.  work: 16 B ceil(H W / 256) + 2 B H W bytes of scratch, 8-byte aligned. */
int s2h_error_center_click(int B, int H, int W, const uint8_t* gt, const uint8_t* pred, float* points, int* labels,
                           int* dmax, void* work, hipStream_t st);
/* P uniformly drawn clicks in the error regions, per object b of B: R0 = FP | (all_correct & ~gt) (label 0), R1 =
 * FN (label 1), all_correct = gt equals pred everywhere; n = |R0| + |R1|.  Click (b, p) is the
 * ((r[b, p] mod 2^32) * n) >> 32 -th pixel of R0 | R1 in row-major order (64-bit product), its label says which set
 * holds it; n = 0: point (0, 0), label 0.  r int64 [B, P] draws in [0, 2^32); points [B, P, 2] fp32 = (x, y);
 * labels [B, P] int32; count [B, 2] int32 = (|R0|, |R1|).  work: 3 B (ceil(H W / 4096) + 1) int32 of scratch. */
int s2h_error_uniform_click(int B, int P, int H, int W, const uint8_t* gt, const uint8_t* pred, const int64_t* r,
                            float* points, int* labels, int* count, int* work, hipStream_t st);
/* Category-merged masks of a tracked frame, bit-packed, without materialising the [N, H, W] logits
 * (reference sam2_video/eval/inference.py:487-514, per object `(out_mask_logits[i] > 0.0).cpu().numpy()` and
 * `torch.sigmoid(out_mask_logits[i]).mean().item()`, and :870-886, the `key % MOD` OR on the host).
 * low [N, hi, wi] fp32 low-res logits; every video-resolution value is the one s2h_bilinear_fwd(N, hi, wi, H,
 * W) computes, bit for bit.  non_overlap: per pixel the object of the highest value keeps it (first index on
 * a tie, torch.argmax), every other object is clamped to <= -10 (upstream
 * _apply_non_overlapping_constraints).  cat_off [Ncat + 1] / cat_obj: the object -> category CSR of
 * s2h_group_max_fwd (an empty category is allowed, a category reads at most N entries).
 * bits [Ncat, ceil(H W / 64)] uint64: bit j % 64 of word j / 64 of a category is set when an object of the
 * category is > 0 (0.0 and -0.0 are background) at pixel (y = j % H, x = j / H): COLUMN-major, the order of
 * COCO RLE; bits past H W are zero.  score [N] = mean over the H W final values of sigmoid(v), fp32, summed in
 * a fixed order (no float atomics: bit-reproducible).  work: N * ceil(H W / 256) fp32 of scratch.
 * H, W >= 1, H * W <= 2^24, Ncat * H * W < 2^31 - 256. */
int s2h_mask_export(int N, int hi, int wi, int H, int W, const float* low, int Ncat, const int* cat_off,
                    const int* cat_obj, int non_overlap, uint64_t* bits, float* score, float* work,
                    hipStream_t st);
/* s2h_mask_export at a tuned threshold: foreground is final value >= cut (NaN is background, -0.0 >= 0.0
 * holds), cut = the logit cut of a float16 probability threshold (reference export_predict_from_probs.py:66,
 * `probs[indices] >= threshold` on float16 sigmoids).  Everything else, score included, as s2h_mask_export.
 * vmax [N] = the maximum over the H W final values of each object, fmaxf from -inf (NaN skipped): the
 * category's score `probs.max()` of the reference is the float16 sigmoid of the maximum over its objects.
 * work: 2 * N * ceil(H W / 256) fp32 of scratch. */
int s2h_mask_export_cut(int N, int hi, int wi, int H, int W, const float* low, int Ncat, const int* cat_off,
                        const int* cat_obj, int non_overlap, float cut, uint64_t* bits, float* score,
                        float* vmax, float* work, hipStream_t st);
/* The threshold sweep of a tracked frame (reference tune_threshold.py:92-110, `np.any(probs[idx] >= thr)` per
 * category and threshold against the ground truth) for K thresholds in one pass, without the [N, H, W] values.
 * low, cat_off, cat_obj, non_overlap and the video-resolution values as for s2h_mask_export.  cuts [K] fp32 on
 * the device, non-decreasing (equal neighbours allowed: their bin stays empty), 1 <= K <= 64.  gt_bits [Ncat,
 * ceil(H W / 64)] uint64: the ground truth per category in the layout s2h_mask_export writes (bits past H W in
 * a last word are ignored); NULL = all background.  Per pixel and category m = the maximum over the category's
 * objects of the final value (NaN skipped, -inf for an empty category) and b = #{k : m >= cuts[k]}.
 * hist [Ncat, 2, K + 1] int32, overwritten: hist[c][g][b] = the pixels with ground-truth bit g in bin b, so
 * every row pair sums to H W and the pixels counting at cut k are the bins above k.  Integer counting (ballot
 * and popcount per wave, integer atomics): a pure function of the inputs, every device loop bounded; sizes as
 * for s2h_mask_export. */
int s2h_mask_sweep(int N, int hi, int wi, int H, int W, const float* low, int Ncat, const int* cat_off,
                   const int* cat_obj, int non_overlap, int K, const float* cuts, const uint64_t* gt_bits,
                   int* hist, hipStream_t st);
/* Run boundaries, area and bounding box of Ncat bit-packed column-major masks (reference inference.py:887-897,
 * `mask.sum()`, maskUtils.encode(np.asfortranarray(mask)) and eval/utils.py:156-165 mask_to_bbox).  A
 * transition is a position j in [0, H W) with m[j] != m[j - 1], m[-1] = 0; the RLE counts are the differences
 * of [0, *transitions, H W].  bits as s2h_mask_export writes them (bits past H W in a last word are ignored).
 * hdr [Ncat, 8] int32 = n_trans, offset, area, xmin, ymin, xmax, ymax (inclusive corners; W, H, -1, -1 for an
 * empty mask), total; trans[offset[c] .. offset[c] + n_trans[c]) = the positions of category c, ascending,
 * the categories back to back.  total = the sum of n_trans = the capacity needed: when it exceeds `capacity`
 * only the first `capacity` positions are written (nothing past the end) and the caller runs again with a
 * larger buffer; the header is complete either way.  work: 7 * Ncat * ceil(ceil(H W / 64) / 256) int32 of
 * scratch.  Integer arithmetic in a fixed order, every device loop bounded; sizes as for s2h_mask_export. */
int s2h_rle_transitions(int Ncat, int H, int W, const uint64_t* bits, int capacity, int* hdr, int* trans,
                        int* work, hipStream_t st);
/* ---- clip loading (reference sam2_video/data/dataset.py:103-110 and :139-179, the torchvision transforms and
 * the pycocotools decode; csrc/preproc.hip).  Both entries are pure functions of their inputs: integer
 * arithmetic, no atomics, no shared memory, no host round trip, every device loop bounded by a table size.
 *
 * Pillow's Image.resize on uint8 RGB, the crop and the normalisation in one call.  src [F, H, W, 3] uint8, all
 * frames one size; out [F, 3, Sh, Sw] fp32.  The filter is in the tables, built on the host per axis (Pillow's
 * precompute_coeffs and normalize_coeffs_8bpc): x_min / x_cnt int32 [Sw] = first source column and tap count of
 * output column o, x_coef int32 [Sw, kx] = the weights * 2^22, rounded; y_* likewise over rows, [Sh] and
 * [Sh, ky].  A cropped output passes only the table rows of its window.  Two passes in Pillow's order:
 * mid[f][r][o][c] = clip8((sum_k x_coef[o][k] * src[f][row0 + r][x_min[o] + k][c] + 2^21) >> 22) for the nrows
 * source rows from row0 (the rows the vertical taps read: every y_min[o] >= row0 and y_min[o] + y_cnt[o] <=
 * row0 + nrows), then the same sum down the columns of mid; out = lut[c][value], lut [3, 256] fp32 filled by
 * the host with the normalised value of every byte.  scratch: F * nrows * Sw * 3 bytes (mid).  A tap window
 * that leaves the line, or is longer than its table row, is cut to what is inside: nothing outside src or
 * scratch is read.  1 <= kx, ky <= 64 (hipErrorInvalidValue otherwise, as for every limit here);
 * 1 <= H, W, Sh, Sw <= 16384; 0 <= row0, row0 + nrows <= H; F * H * W * 3, F * nrows * Sw * 3 and
 * F * 3 * Sh * Sw < 2^31 - 256. */
int s2h_resample_u8_norm(int F, int H, int W, const uint8_t* src, int Sw, int kx, const int* x_min,
                         const int* x_cnt, const int* x_coef, int Sh, int ky, const int* y_min, const int* y_cnt,
                         const int* y_coef, int row0, int nrows, const float* lut, uint8_t* scratch, float* out,
                         hipStream_t st);
/* Category masks of F frames from COCO RLE, nearest-resized and cropped, without the dense H x W masks.
 * run_off [A + 1] / run_end as for s2h_rle_decode, the A annotations of all frames back to back, every one
 * of an H x W image; ann_cat [A] int32 = the category index of an annotation, outside [0, N) = skipped;
 * frame_off [F + 1] = the annotations of frame f are [frame_off[f], frame_off[f + 1]) (cut to [0, A]).
 * row_map [Sh] / col_map [Sw] int32 = the source row / column of each output row / column (the nearest resize
 * and the crop folded in by the host; values in [0, H) / [0, W)).  out [F, N, Sh, Sw] uint8 of 0 / 1, every
 * element written: out[f][n][y][x] = OR over frame f's annotations of category n of k & 1, k = the number of
 * the annotation's run_end <= col_map[x] * H + row_map[y] (binary search, at most 32 steps).
 * 0 <= N <= 64; 1 <= H, W, Sh, Sw <= 16384; H * W and F * N * Sh * Sw < 2^31 - 256. */
int s2h_rle_catmasks(int F, int N, int H, int W, int A, const int* run_off, const int* run_end,
                     const int* ann_cat, const int* frame_off, int Sh, int Sw, const int* row_map,
                     const int* col_map, uint8_t* out, hipStream_t st);
/* ---- dataset preparation (reference data/convert_endovis_to_coco.py:132-179 and
 * data/apply_morphological_opening.py:57-72; csrc/dataprep.hip).  Both entries are pure functions of their inputs:
 * integer arithmetic, no float, no 64-bit atomics, no host round trip, every device loop bounded by the sizes.
 * Limits of s2h_rle_decode and s2h_rle_transitions: H, W >= 1, H * W <= 2^24, F * H * W and P * H * W
 * < 2^31 - 256 (hipErrorInvalidValue otherwise).
 *
 * Per frame the pixel count of every byte value (np.unique / np.bincount of a label image).  labels [F, H, W]
 * uint8, row-major; hist [F, 256] int32, zeroed by the call.  32-bit counters privatised per workgroup in LDS,
 * then one integer atomic per non-zero counter. */
int s2h_label_hist(int F, int H, int W, const uint8_t* labels, int* hist, hipStream_t st);
/* Row-major label bytes -> the column-major bit words s2h_rle_transitions reads, one plane per (frame, class).
 * Plane p belongs to frame f when frame_off[f] <= p < frame_off[f + 1] (frame_off [F + 1], CSR, ascending from 0
 * to P); bits [P, ceil(H W / 64)]: bit j % 64 of word j / 64 of plane p = (labels[f][j % H][j / H] ==
 * plane_class[p]), or (labels[f][j % H][j / H] != 0) when plane_class[p] == -1 (byte masks, e.g. after
 * s2h_morph_rect: one frame and one plane per mask).  The layout is s2h_mask_export's; bits past H W are zero.
 * Every word of every plane is written exactly once, and no plane outside [0, P) whatever frame_off holds.
 * P == 0 returns without a launch.  A workgroup stages one frame's band of 64 columns in LDS (H * 64 bytes,
 * H <= 2048) and builds every plane of the frame from it; taller images are read straight from memory. */
int s2h_label_planes(int F, int H, int W, const uint8_t* labels, int P, const int* frame_off,
                     const int* plane_class, uint64_t* bits, hipStream_t st);
/* ---- training visualisation (reference utils/viz.py; csrc/viz.hip, the picture is csrc/viz_pixel.h).  Pure
 * functions of their inputs, integer arithmetic but for the frame conversion (two separately rounded double
 * operations), no atomics, no host round trip, one launch each whatever the data holds.
 * Limits of both: 1 <= H, W; 1 <= C <= 64; n * 2H * 2W * 3 < 2^31 (hipErrorInvalidValue otherwise); n == 0
 * returns without a launch.
 *
 * Category words: words [n, H W] uint64, bit c of words[f][p] = (src[f][c][p] > 0.5) -- the reference's rule for
 * ground truth and raw logits alike.  kind 0: src uint8 / bool (set = non-zero), kind 1: fp32 (NaN = clear).
 * Frame f's [C, H, W] block starts frame_stride elements after frame f - 1's (>= 0; C H W = contiguous frames), so
 * every k-th frame of a clip is read where it lies.  Every word is written exactly once. */
int s2h_viz_pack(int n, int C, int H, int W, int kind, const void* src, int64_t frame_stride, uint64_t* words,
                 hipStream_t st);
/* The n composites: out [n, 2H, 2W, 3] uint8 (4-byte aligned), every byte written exactly once, in whole dwords.
 * Panels: top-left frame f, top-right frame f + the overlay of gt_words[f], bottom-left frame0 + prompts,
 * bottom-right frame f + the overlay of pred_words[f].
 * img_kind 0: frames fp32 [3, H, W] per frame, ImageNet-normalised, u = trunc(clamp((double)x * std_c + mean_c, 0, 1)
 * * 255) (NaN -> 0); img_kind 1: uint8 [H, W, 3] passed through.  frame_stride (elements) as for s2h_viz_pack;
 * frame0 = one frame of the same kind.
 * Overlay panel: every pixel (4 base + overlay + 2) / 5 per channel with overlay = palette[highest set category]
 * or 0 (cv2.addWeighted(base, 0.8, overlay, 0.2), pixels without a mask included); then, at full opacity,
 * palette[highest category c whose 3 x 3 neighbourhood, positions outside the image ignored, holds both a pixel
 * with c set and one with c clear].  palette [C, 3] uint8.
 * Prompts: prompt_words [H W] non-null (mask prompts) = frame0 with that overlay, no markers.  Otherwise the M <= 256
 * markers [M, 8] int32 {kind, x1, y1, x2, y2, r, g, b} in table order, later ones overwriting, clipped to the
 * image: kind 0 disc at (x1, y1) -- colour where dx^2 + dy^2 < 49, white where 49 <= dx^2 + dy^2 <= 81; kind 1
 * cross -- (|dx| <= 1 and |dy| <= 8) or (|dy| <= 1 and |dx| <= 8); kind 2 box -- x1 <= x <= x2, y1 <= y <= y2 and
 * min(x - x1, x2 - x, y - y1, y2 - y) < 2 (an inverted box paints nothing); other kinds paint nothing. */
int s2h_viz_compose(int n, int C, int H, int W, int img_kind, const void* frames, int64_t frame_stride,
                    const void* frame0, const uint64_t* gt_words, const uint64_t* pred_words,
                    const uint64_t* prompt_words, const uint8_t* palette, int M, const int* markers, uint8_t* out,
                    hipStream_t st);
/* The first upscaling step in one pass (mask_decoder.py:105-106, bf16, Co = 64): pre = the s2h_convt2_store
 * values, y / mean / rstd = LayerNorm2d(pre) over the channels (gamma, beta, eps; the values of
 * s2h_layernorm_fwd), post = gelu(y) (as s2h_act_fwd rounds it); mean / rstd [B * 2H * 2W] fp32. */
int s2h_convt2_ln_gelu(int dt, int B, int H, int W, int Co, const void* Y, const float* bias, const void* add,
                       int add_bcast, const float* gamma, const float* beta, float eps, void* pre, void* y,
                       float* mean, float* rstd, void* post, hipStream_t st);
/* y[r, :] = gate[r] > 0 ? x[r, :] : fill; dir 1 = backward (object-score gating to
 * NO_OBJ_SCORE, sam2_base.py:380-389). */
int s2h_row_gate(int dt, int64_t rows, int64_t inner, const void* x, const float* gate, float fill,
                 void* y, int dir, hipStream_t st);
/* s2h_row_gate with input type dt_in and output type dt_out (the low-res mask logits' cast to fp32
 * fused with the gate; its backward back to bf16); gate_out (nullable): gate[0:rows] copied. */
int s2h_row_gate_cast(int dt_in, int dt_out, int64_t rows, int64_t inner, const void* x, const float* gate,
                      float fill, void* y, int dir, float* gate_out, hipStream_t st);
/* y = (scale_x ? g*x : x) + (1-g)*vec for g = (gate > 0) (obj_ptr / no_obj_ptr mix,
 * sam2_base.py:413-424; no_obj_embed_spatial sam2_base.py:761-767). */
int s2h_gate_mix(int dt, int64_t rows, int64_t inner, const void* x, const float* gate, const void* vec,
                 int vec_period, int scale_x, void* y, hipStream_t st);
/* Hiera positional embedding: out[h, w, c] = Y[c, h, w] + win[c, h % ws, w % ws]
 * (bicubic-resized background + tiled window embedding, hieradet.py:273-281). */
int s2h_pos_embed(int dt, int C, int h, int w, int ws, const float* Y, const float* win, void* out,
                  hipStream_t st);
int s2h_pos_embed_bwd(int dt, int C, int h, int w, int ws, const void* dout, float* dY, float* dwin,
                      hipStream_t st);
/* Point prompt embedding: out[r] = pe[r] + table[label[r] + 1] (label -1 = pad:
 * table row 0 = not_a_point_embed, pe zeroed), prompt_encoder.py:79-104; labels_out (nullable):
 * the labels copied (kept for the backward). */
int s2h_point_embed(int dt, int R, int D, const float* pe, const int* labels, const void* table, void* out,
                    int* labels_out, hipStream_t st);
int s2h_point_embed_bwd(int dt, int R, int D, const int* labels, const void* dout, float* dtable, hipStream_t st);
/* the same with the 5 label rows' gradients at their own addresses (host array of 5 fp32 [D] rows:
 * not_a_point_embed, point_embeddings[0..3] -- the parameters' arena gradients), accumulated in row order. */
int s2h_point_embed_bwd_rows(int dt, int R, int D, const int* labels, const void* dout, float* const* drows,
                             hipStream_t st);

/* ---------------------------------------------------------------- loss + category merge
 * Per-row mask statistics of logits x/T vs uint8 targets: stats[6*r..] = (focal sum,
 * sigmoid sum, target sum, sigmoid.target sum, (x>0) & tgt count, (x>0) | tgt count).
 * sigmoid_focal_loss / dice_loss / iou_loss inputs, losses.py:20-76, 111-248. */
int s2h_mask_stats(int N, int64_t P, const float* x, int64_t ldx, const uint8_t* tgt, int64_t ldt,
                   float inv_temp, float* stats, hipStream_t st);
/* losses[4] = (loss_mask, loss_dice, loss_iou, weighted total) with per-frame
 * normalisation by valid categories (valid = NULL: target sum > 0); losses is added to.
 * coef[4*N] are the gradient coefficients consumed by s2h_mask_loss_bwd, four per row:
 * [0] the focal coefficient gscale w_mask / (nv P), [1] Dice A = gscale w_dice 2 / (nv den),
 * [2] Dice B = gscale w_dice (2 sum(sigma t) + 1) / (nv den^2) with den = sum sigma + sum t + 1,
 * [3] d total / d pred_iou = gscale w_iou sign(pred_iou - actual) / nv; zeros on an invalid row.
 * A frame with no valid row leaves losses unchanged and writes an all-zero coef. */
int s2h_mask_loss_finalize(int N, int64_t P, const float* stats, const float* pred_iou, const int* valid,
                           float w_mask, float w_dice, float w_iou, float gscale, float* losses,
                           float* coef, hipStream_t st);
/* dx = d(total)/d(logits) * gtot[3] (device scalar upstream gradient, NULL = 1); dious likewise
 * (may be NULL).  tgt is required: NULL is refused with hipErrorInvalidValue before any launch. */
int s2h_mask_loss_bwd(int N, int64_t P, const float* x, int64_t ldx, const uint8_t* tgt, int64_t ldt,
                      float inv_temp, const float* coef, float* dx, int64_t lddx, const float* gtot,
                      float* dious, hipStream_t st);
/* BCECategoryLoss (losses.py:251-372, loss.type=bce): per-row stats[2*r..] = (sum of
 * binary_cross_entropy_with_logits(x/T, t, pos_weight[r]), target sum); pos_weight may be NULL. */
int s2h_bce_stats(int N, int64_t P, const float* x, int64_t ldx, const uint8_t* tgt, int64_t ldt,
                  float inv_temp, const float* pos_weight, float* stats, hipStream_t st);
/* losses[0] += frame_scale * (mean (reduction 0) or sum (1) over the rows with target pixels);
 * coef[N] are the backward coefficients. */
int s2h_bce_finalize(int N, int64_t P, const float* stats, int reduction, float frame_scale, float* losses,
                     float* coef, hipStream_t st);
/* dx = gtot[0] * d(loss)/d(logits) (gtot: device scalar upstream gradient, NULL = 1). */
int s2h_bce_bwd(int N, int64_t P, const float* x, int64_t ldx, const uint8_t* tgt, int64_t ldt, float inv_temp,
                const float* pos_weight, const float* coef, const float* gtot, float* dx, int64_t lddx,
                hipStream_t st);
/* Evaluation counts of one frame (eval/eval.py:16-40 caculate_iou / _dice / _mae on the
 * binarised category-merged mask pred = logits > 0): counts[4n..4n+3] = |pred & gt|,
 * |pred | gt|, |pred|, |gt| as uint64 (zeroed by the call).  Validation only, no gradient. */
int s2h_mask_eval_counts(int N, int64_t P, const float* x, int64_t ldx, const uint8_t* tgt, int64_t ldt,
                         uint64_t* counts, hipStream_t st);
/* Pixelwise max of each category's object masks (CSR cat_off / cat_obj), argmax
 * saved for the backward (merge_object_results_to_category, masks.py:98-115). */
int s2h_group_max_fwd(int Ncat, int64_t P, const int* cat_off, const int* cat_obj, const float* x,
                      int64_t ldx, float* y, int64_t ldy, int* arg, hipStream_t st);
int s2h_group_max_bwd(int O, int64_t P, const int* obj_cat, const int* arg, const float* dy, int64_t lddy,
                      float* dx, int64_t lddx, hipStream_t st);
/* Sigmoid-mass weighted mean of per-object scalars (IoU / object scores) per
 * category, weights = stats (masks.py:98-140); bwd also yields d(weights). */
int s2h_group_wavg_fwd(int Ncat, int K, const int* cat_off, const int* cat_obj, const float* stats,
                       const float* x, float* y, hipStream_t st);
int s2h_group_wavg_bwd(int O, int K, const int* obj_cat, const int* cat_off, const float* stats,
                       const float* x, const float* y, const float* dy, float* dx, float* dw, hipStream_t st);
/* dx[r, :] += coef[r] * sigmoid'(x[r, :]) (gradient of the sigmoid-mass weights). */
int s2h_sigmoid_grad_axpy(int R, int64_t P, const float* x, int64_t ldx, const float* coef, float* dx,
                          int64_t lddx, hipStream_t st);

/* ---------------------------------------------------------------- optimizer
 * Global L2 norm of the flat fp32 gradient arena (times grad_scale) and the clip
 * factor: out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6)) * grad_scale.
 * partial_ws: fp32 workspace of >= 1024 floats.  Replaces gradient_clip_val
 * (torch clip_grad_norm_, configured at trainer / best.yaml:106). */
int s2h_grad_norm(int64_t n, const float* g, float* partial_ws, float max_norm, float grad_scale,
                  float* out, hipStream_t st);
/* Fused AdamW over the flat arena (torch.optim.AdamW semantics, trainer.py:125):
 * g' = g*clip[1]; p *= 1 - lr*wd; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 * p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps); optional bf16 shadow copy. */
int s2h_adamw(int64_t n, float* p, const float* g, float* m, float* v, const float* clip, float lr,
              float beta1, float beta2, float eps, float wd, int step, void* bf16_shadow, hipStream_t st);
/* Stochastic weight averaging over the flat master arena (Lightning's StochasticWeightAveraging.avg_fn with its
 * device-tensor divisor).  s2h_swa_update: n_averaged == 0 copies p into avg; otherwise
 * avg = avg + (p - avg) / (float)(n_averaged + 1) in fp32 -- a subtraction, a correctly rounded IEEE division (no
 * reciprocal) and an addition, each rounded once.  s2h_swa_apply: p = avg and, when bf16_shadow is not NULL, the
 * shadow in the rounding of s2h_adamw / s2h_cast.  Both write in place (captured graphs that read p or the
 * shadow stay valid); n elements, 16-B accesses when the pointers are 16-B (shadow: 8-B) aligned. */
int s2h_swa_update(int64_t n, float* avg, const float* p, int n_averaged, hipStream_t st);
int s2h_swa_apply(int64_t n, const float* avg, float* p, void* bf16_shadow, hipStream_t st);

/* ---------------------------------------------------------------- prompt stage (host CPU code)
 * The per-step host work of prepare_prompt_inputs (sam2model.py:181-236) on frame 0, native and
 * multi-threaded (one thread per category, `threads` at most); no device calls.
 * s2h_prompt_objects replaces cat_to_obj_mask + find_connected_components (masks.py:13-50, the
 * cv2 5x5-ellipse opening + 8-connected components): N category masks [N, H, W] of 0/1 bytes ->
 * objects numbered category-major, raster order of first pixel within a category; obj_cat[o],
 * stats[o * 7 ..] = (count, sum_y, sum_x, y_min, y_max, x_min, x_max), optional lab[N, H, W] =
 * 1 + object index (0 background).  Returns 0, 2 with *n_obj = the count needed when it
 * exceeds max_obj, 1 on bad arguments.
 * s2h_prompt_object_masks: lab -> float object masks [n_obj, H, W] (cat_to_obj_mask's output).
 * s2h_mask_moments: the same 7 moments of B whole masks [B, H, W] -- the centre-of-mass click of
 * generate_point_prompt (prompts.py:13-75) and the corners of generate_box_prompt (prompts.py:78-97). */
int s2h_prompt_objects(int N, int H, int W, const uint8_t* masks, int max_obj, int* n_obj, int32_t* obj_cat,
                       int64_t* stats, int32_t* lab, int threads);
int s2h_prompt_object_masks(int N, int H, int W, const int32_t* lab, int n_obj, float* out, int threads);
int s2h_mask_moments(int B, int H, int W, const uint8_t* masks, int64_t* stats, int threads);

#ifdef __cplusplus
}
#endif

#endif /* SAM2HIP_H */
