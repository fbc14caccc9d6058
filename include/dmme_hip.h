/*
 * dmme_hip.h -- C ABI of libdmme_hip.so: the MI355X (gfx950) denoiser hot path.
 *
 * The reference (urw7rs/diffusion-models-made-easy v0.5.2) is pure Python and has no
 * FFI of its own; every entry point below replaces a *Python* interface of the hot
 * path and cites it (paths relative to the reference root).  A maintainer binds these
 * with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; no torch / C++ types cross the boundary;
 *   - every device pointer is caller-owned (the plan never owns tensor memory; it
 *     owns host metadata plus one small device table used by the weight re-packer);
 *   - every call is asynchronous on the caller's HIP stream (`stream` is a
 *     hipStream_t passed as void*); no hidden synchronisation or allocation in the
 *     launch path, so calls can be captured into a hipGraph;
 *   - return value: 0 (DMME_OK) or a negative dmme_status; the message of the last
 *     failure on the calling thread is available from dmme_last_error();
 *   - no exceptions cross the ABI.
 *
 * Tensor layouts at the boundary
 *   - images x / y / eps / z: NCHW fp32 (what the reference's UNet.forward takes,
 *     src/dmme/models/ddpm.py:281-316);
 *   - timesteps: int64 device array of length 1 or B (reference passes `all_t[t]`
 *     of shape (1,) when sampling, (B,) when training; diffusion_models/ddpm.py:65-77,124-131);
 *   - parameters: one flat fp32 buffer in reference state_dict order and reference
 *     layouts (conv OIHW, linear (out,in)); dmme_unet_pack_params() converts it to
 *     the library's packed layout ([Cout][kh][kw][Cin], compute dtype).
 */
#ifndef DMME_HIP_H
#define DMME_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(DMME_BUILD)
#define DMME_API __attribute__((visibility("default")))
#else
#define DMME_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DMME_OK = 0,
    DMME_ERR_INVALID = -1,     /* bad argument / shape the reference would also reject */
    DMME_ERR_UNSUPPORTED = -2, /* valid in the reference, not supported by this build */
    DMME_ERR_HIP = -3,         /* a HIP runtime call failed */
    DMME_ERR_NOMEM = -4
} dmme_status;

/* DMME_BF16X3: the accurate mode.  Tensors and weights stay fp32 (same layouts, workspace and packed sizes as DMME_F32); every
 * convolution product runs as three bf16 MFMA passes over hi/lo splits of its fp32 operands (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi,
 * fp32 accumulation), ~2^-16 per product instead of 2^-9: within 1e-3 of the fp32 reference at the bf16 matrix rate / 3.
 * Accepted wherever a dtype is (plans and the single-op entry points); buffers are the fp32 ones. */
/* DMME_F16R32: the reduced-precision mode that stays within 1e-3 of the fp32 reference (precision="fp16r32", inference).  A
 * DMME_F16 plan whose FULL-RESOLUTION level - where a rounding error reaches the output undamped: the first and last ResBlocks,
 * the skip tensors between them, input and output conv (models/ddpm.py:293-295, 308-315) - keeps its tensors in fp32 and runs
 * every product as three fp16 MFMA passes over hi / lo halves of both operands (csrc/conv_pipe.hip: conv3x3_ws2_kernel<.., SPLIT>);
 * every level below it is plain DMME_F16.  Workspace and packed sizes differ from DMME_F16's (query them). */
typedef enum { DMME_F32 = 0, DMME_BF16 = 1, DMME_BF16X3 = 2, DMME_F16 = 3, DMME_F16R32 = 4 } dmme_dtype;

/* Which of the reference's two UNets the plan builds. */
typedef enum {
    DMME_ARCH_DDPM = 0,  /* dmme.models.ddpm.UNet (src/dmme/models/ddpm.py:176-316): eps only */
    DMME_ARCH_IDDPM = 1, /* dmme.models.iddpm.UNet (src/dmme/models/iddpm.py:125-265): scale-shift ResBlocks,
                            multi-head attention, 2*in_channels outputs (eps, v) */
    DMME_ARCH_CLASSIFIER = 2, /* the noise-aware classifier of classifier guidance (Dhariwal & Nichol 2021, the ADM "half UNet";
                            the reference's src/dmme/guidance/classifier.py sketch): the DDPM UNet's time MLP, input_conv,
                            down_layers and middle_layers (same keys and layouts), then the head `out` = GroupNorm -> SiLU ->
                            mean over H x W -> Linear(C_top, num_classes).  No up path, no output conv.  The output y is the
                            fp32 logits (B, num_classes).  fp32 / bf16 / fp16 only (bf16x3 / fp16r32: DMME_ERR_UNSUPPORTED);
                            per-op launches (no level engine); no gradient buckets. */
    DMME_ARCH_DDPM_COND = 3 /* the DDPM UNet with a class label (classifier-free guidance, Ho & Salimans 2021; conditioning in the ADM form,
                            Dhariwal & Nichol 2021): DMME_ARCH_DDPM's parameter table, unchanged, plus ONE entry behind it,
                            `label_emb.weight` (num_classes + 1, emb_dim), fp32 in the packed buffer; row num_classes is the null label.  The
                            label row enters the pre-activation of the second time Linear: c_b = SiLU(W2 h1_r + b2 + E[y_b]), r = b for
                            t_len == B and 0 for t_len == 1; from the per-block projection on the forward runs with B time rows whatever
                            t_len was.  Routes, level engine, residual segments and gradient buckets are DMME_ARCH_DDPM's (the table's
                            gradient rides in the last bucket).  fp32 / bf16 / fp16 only (bf16x3 / fp16r32: DMME_ERR_UNSUPPORTED).  Runs
                            through the dmme_*_cond entry points only: the label-less ones return DMME_ERR_INVALID on such a plan. */
} dmme_unet_arch;

/* Constructor arguments of the reference UNet (src/dmme/models/ddpm.py:190-200, models/iddpm.py:139-149). */
typedef struct {
    int in_channels;
    int pos_dim;
    int emb_dim;
    int num_groups;
    float dropout;
    int num_depths;
    int channels_per_depth[8];
    int num_blocks;
    int num_attention_depths;
    int attention_depths[8];
    int arch;      /* dmme_unet_arch */
    int num_heads; /* DMME_ARCH_IDDPM: heads of MultiHeadAttention (the reference hard-codes 4, models/iddpm.py:82);
                      ignored (1) for DMME_ARCH_DDPM */
    int num_classes; /* DMME_ARCH_CLASSIFIER: classes of the head (>= 1); DMME_ARCH_DDPM_COND: classes K of the label table (>= 1);
                        ignored otherwise */
} dmme_unet_cfg;

typedef struct dmme_plan dmme_plan;

DMME_API const char* dmme_last_error(void);
DMME_API int dmme_version(void);
/* number of HIP devices visible to the library (0 => the library loaded but cannot compute) */
DMME_API int dmme_device_count(void);

/* ---- UNet plan: replaces UNet.__init__ (models/ddpm.py:190-279) --------------------
 * Builds the layer graph (including the reference's always-false `if` at :242), the
 * parameter table, the packed-weight layout and the activation workspace layout for a
 * fixed (B, H, W, dtype).  Host-only arithmetic, the backward's tables included; `device` selects which GPU
 * owns the plan's small device tables (-1: do not touch any device, for CPU-side inspection: such a plan
 * reports the same gradient buckets, dmme_unet_plan_bwd_summary and backward workspace size as a device
 * plan of the same arguments on a device that holds the default number of resident level-engine
 * workgroups, and cannot launch). */
DMME_API int dmme_unet_plan_create(const dmme_unet_cfg* cfg, int B, int H, int W, int dtype, int device, dmme_plan** out);
DMME_API void dmme_unet_plan_destroy(dmme_plan* plan);

/* Parameter table in reference state_dict order (305 entries for the default config;
 * SURVEY 8b).  `ref_offset` is the element offset inside the flat fp32 buffer. */
DMME_API int dmme_unet_plan_num_params(const dmme_plan* plan);
DMME_API int dmme_unet_plan_param_info(const dmme_plan* plan, int index, char* name, int name_cap, int* ndim,
                              int64_t shape[4], int64_t* ref_offset, int* is_buffer);
DMME_API int64_t dmme_unet_plan_ref_numel(const dmme_plan* plan);
DMME_API int64_t dmme_unet_plan_packed_bytes(const dmme_plan* plan);
DMME_API int64_t dmme_unet_plan_workspace_bytes(const dmme_plan* plan);
/* floats in a full set of Dropout2d multipliers: sum over ResBlocks of B*Cout, laid out
 * block after block (graph order: down, middle, up), each [B][Cout]. */
DMME_API int64_t dmme_unet_plan_dropmask_numel(const dmme_plan* plan);
/* channels of the network output: in_channels (DDPM) or 2*in_channels (IDDPM: eps and v stacked) */
DMME_API int dmme_unet_plan_out_channels(const dmme_plan* plan);
/* number of kernel launches one forward issues (for launch-overhead accounting) */
DMME_API int dmme_unet_plan_num_launches(const dmme_plan* plan);
/* ... of dmme_unet_forward_nograd / dmme_chain_step with every foldable attention block folded (dmme_unet_pack_folded): one launch
 * fewer per such block.  dmme_unet_plan_num_launches and dmme_unet_plan_op_info describe the form a backward pass can follow.
 * dmme_unet_plan_num_folded: how many blocks that is (0: nothing to fold - other batch sizes, precisions, DMME_NO_ATTN_FOLD). */
DMME_API int dmme_unet_plan_num_launches_nograd(const dmme_plan* plan);
DMME_API int dmme_unet_plan_num_folded(const dmme_plan* plan);

/* fp32 reference-layout flat buffer -> packed buffer (replaces nothing in the
 * reference; it is the load_state_dict side of the boundary).  Ends the validity of this buffer's folded slots (below). */
DMME_API int dmme_unet_pack_params(const dmme_plan* plan, const float* ref_flat, void* packed, void* stream);
/* Once per weight version, behind dmme_unet_pack_params on the same stream and ahead of no-grad forwards / chain steps: the folded
 * matrices of the single-head 16x16 attention blocks (M = C^-0.5 Wk^T Wq, c = C^-0.5 Wk^T bq, Wpv = Wp Wv, b' = Wp bv + bp; fp32 sums
 * over the 16-bit weights in `packed`, one rounding) into their slots of `packed` (dmme_unet_plan_packed_bytes covers them).  From
 * then until the next dmme_unet_pack_params of that buffer, dmme_unet_forward_nograd, dmme_chain_step and dmme_unet_forward_profiled
 * with that buffer run those blocks without a qkv conv or tensor (dmme_attention_block).  Without this call, or with another buffer,
 * they run the unfolded walk.  A captured graph holds the walk it was captured with.  A backward-capable forward never folds. */
DMME_API int dmme_unet_pack_folded(const dmme_plan* plan, void* packed, void* stream);

/* ---- UNet forward: replaces UNet.forward (models/ddpm.py:281-316) -------------------
 * y = eps_theta(x, t).  x: (B, C, H, W), y: (B, dmme_unet_plan_out_channels(), H, W), fp32 NCHW.
 * t: int64[t_len], t_len in {1, B}.  DMME_ARCH_IDDPM: iddpm.UNet.forward (models/iddpm.py:232-265).
 * drop_masks: NULL for eval(); else the Dropout2d multipliers (0 or 1/(1-p)) laid out
 * as dmme_unet_plan_dropmask_numel() describes (nn.Dropout2d, models/ddpm.py:29). */
DMME_API int dmme_unet_forward(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len,
                      float* y, void* workspace, const float* drop_masks, void* stream);
/* The same forward where no dmme_unet_backward will follow (the reference's sampling loops run under torch.no_grad(),
 * diffusion_models/ddpm.py:113-133): tensors that only the backward pass reads - the context of an attention block whose proj
 * conv runs inside the attention launch (models/ddpm.py:66-75), raw conv outputs of the level engine that only their norm's
 * pre-activated copy stands for - are not written.  Same arguments, same result y.  dmme_unet_backward on that workspace fails
 * with DMME_ERR_INVALID until a dmme_unet_forward has filled it again.  A REPLAYED graph of this form passes through no entry point:
 * the forward's first launch leaves a mark in the workspace, and a dmme_unet_backward enqueued after such a replay (with no
 * dmme_unet_forward in between) finds it on the device, writes NaN into every gradient it produces and raises the plan's status word,
 * so that dmme_unet_plan_check (and the next entry point) fails with DMME_ERR_INVALID naming this form.
 * dmme_chain_step and dmme_unet_forward_profiled run this form. */
DMME_API int dmme_unet_forward_nograd(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len,
                      float* y, void* workspace, const float* drop_masks, void* stream);

/* ---- class-conditional forward / backward (DMME_ARCH_DDPM_COND plans) -----------------------------------------------
 * labels: int64[B] on the device, values in [0, K]; K = cfg.num_classes is the null label.  The argument check cannot see device labels:
 * a label outside [0, K] is clamped before it indexes the table, that image's time-embedding row (and with it its output) becomes NaN
 * and *status (nullable, device int) is set to 1, as by dmme_log_softmax_grad.
 * dmme_unet_forward_cond: dmme_unet_forward (keep_ctx != 0: a backward may follow) or dmme_unet_forward_nograd (keep_ctx == 0).
 * dmme_unet_backward_cond: dmme_unet_backward_buckets with the labels of the matching forward; `ready` may be NULL (no hand-overs:
 *   dmme_unet_backward).  Adds dE[k] += sum_{b: y_b = k} d z2[b] into grad_flat at the table's ref_offset, summed in ascending b by one
 *   workgroup per row (no atomics: equal inputs give equal bits; a row no image carries is not touched).  Parameter gradients need one
 *   time row per image: t_len == 1 with B > 1 is DMME_ERR_INVALID.
 * dmme_unet_backward_input_cond: dmme_unet_backward_input on a conditional plan (the labels only say which forward it follows). */
DMME_API int dmme_unet_forward_cond(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len, const int64_t* labels,
                                    float* y, void* workspace, const float* drop_masks, int keep_ctx, int* status, void* stream);

/* ---- per-op accounting + event-bracketed profiling (bench.py's roofline leg) --------
 * op_info: kernel label (the kernel symbol the op launches, e.g.
 * "conv_mfma_kernel<bf16,9,128,128>"), its algorithmic FLOPs and algorithmic HBM bytes
 * (every operand read once, result written once) for the plan's (B,H,W).
 * forward_profiled: same launches as dmme_unet_forward, but each op is bracketed by HIP
 * events on `stream`; synchronises, then writes one elapsed time per op (ms). */
DMME_API int dmme_unet_plan_num_ops(const dmme_plan* plan);
/* Level-engine launches of this plan (csrc/lvl_engine.hip: one persistent launch per stretch of layers on a 4x4 / 8x8 map, replacing
 * the per-layer launches of ResBlock / Attention there, models/ddpm.py:118-133, 38-75) as text: "runs=N [map=4x4 plan_ops=a-b
 * engine_ops=.. groups=.. per_iteration=.. workgroups=.. epoch=.. err=..] ...".  err != 0: a bounded in-kernel wait timed out (results of
 * that launch are invalid).  Synchronises with the device (reads the control words). */
DMME_API int dmme_unet_plan_level_info(const dmme_plan* plan, char* buf, int cap);
/* Status of the level engine's bounded hand-off waits.  The engine's workgroups exchange tensors through spin-waits, so all of a
 * launch must be resident at once (the plan sizes its grids by what the device holds and keeps per-op launches otherwise); a wait
 * that still times out - compute units held by another stream, process or CU mask - lets the launch drain with invalid numbers and
 * raises a host-visible status word.  dmme_unet_forward / _forward_profiled / _backward / dmme_chain_step look at that word on
 * entry and fail with DMME_ERR_HIP (clearing it); this call is for hosts that REPLAY a captured graph of those launches (no entry
 * point runs then): call it after synchronising with the stream, before using the results.  DMME_OK: every engine launch of this
 * plan completed since the last check.  (Own invariant of the MI355X path; the reference's loop it guards:
 * src/dmme/diffusion_models/ddpm.py:113-133.) */
DMME_API int dmme_unet_plan_check(const dmme_plan* plan);
DMME_API int dmme_unet_plan_op_info(const dmme_plan* plan, int index, char* label, int label_cap, double* flops,
                           double* bytes);
DMME_API int dmme_unet_forward_profiled(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t,
                               int t_len, float* y, void* workspace, const float* drop_masks, void* stream,
                               float* op_ms);

/* ---- training: replaces loss.backward() through the UNet + the optimiser side of the step ----
 * dmme_unet_backward: given d_y = dL/d(eps) (NCHW fp32) and the workspace left by the matching
 * dmme_unet_forward call (same x, t, drop_masks), ACCUMULATES dL/d(parameters) into grad_flat
 * (fp32, reference state_dict order and layouts, like the flat parameter buffer).
 * packed_bwd holds transposed, tap-flipped conv weights (dmme_unet_pack_params_bwd) for the
 * data-gradient convolutions. Replaces torch autograd of models/ddpm.py:281-316.
 * d_x (nullable): when given, receives dL/dx (NCHW fp32, shape of x) - the gradient autograd hands back for an input that
 * requires grad (guidance-style callers); NULL skips that convolution. */
DMME_API int64_t dmme_unet_plan_packed_bwd_bytes(const dmme_plan* plan);
DMME_API int64_t dmme_unet_plan_bwd_workspace_bytes(const dmme_plan* plan);
DMME_API int dmme_unet_pack_params_bwd(const dmme_plan* plan, const float* ref_flat, void* packed_bwd, void* stream);
DMME_API int dmme_unet_backward(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x,
                       const int64_t* t, int t_len, const float* d_y, void* workspace, void* bwd_workspace,
                       const float* drop_masks, float* grad_flat, float* d_x, void* stream);
/* Same backward in GRADIENT BUCKETS, so a data-parallel caller can exchange a bucket while the rest of backward is still being
 * computed (north star: "RCCL all-reduce of UNet grads over xGMI overlapped with backward"; the reference gets this from
 * Lightning's DDP wrapper around `loss.backward()`, 25 MB buckets).  The op list is cut at ResBlock boundaries into stretches of
 * at most ~1/6 of the parameters, in the order backward finishes them: output conv + the last up blocks first, ..., the first down
 * blocks + input conv + time MLP last (<= 15 % of the bytes: the only exchange nothing can hide).  `ready(user, bucket, offset,
 * numel)` is called on the calling thread - once per contiguous range of a bucket (a bucket may cover two: middle_layers and
 * output_conv sit behind up_layers in the flat buffer) - as soon as every launch that writes grad_flat[offset, offset + numel) has
 * been ENQUEUED on `stream` (record an event there; nothing has necessarily executed yet).  Same results as dmme_unet_backward.
 * dmme_unet_plan_grad_buckets: the (offset, numel, bucket) triples in hand-over order, returns their count (may exceed `cap`);
 * 1 = the configuration has no clean cut, `ready` is then never called. */
typedef void (*dmme_bucket_fn)(void* user, int bucket, int64_t offset, int64_t numel);
DMME_API int dmme_unet_backward_buckets(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x,
                               const int64_t* t, int t_len, const float* d_y, void* workspace, void* bwd_workspace,
                               const float* drop_masks, float* grad_flat, float* d_x, void* stream, dmme_bucket_fn ready, void* user);
/* The input gradient alone: the same backward pass as dmme_unet_backward, but only d_x (required) is written.  No weight-gradient
 * launch runs (grouped or per-layer weight gradients, column sums, bias / time-projection reductions, the packed-image unpack, the
 * time-MLP backward) and grad_flat does not exist here: what a guidance step needs, d log p(y | x_t, t) / d x_t, without paying for
 * the parameters' gradients.  Either architecture (a DMME_ARCH_CLASSIFIER plan takes d_y = d logits, (B, num_classes) fp32).  No host
 * synchronisation: capturable. */
DMME_API int dmme_unet_backward_input(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t,
                                      int t_len, const float* d_y, void* workspace, void* bwd_workspace, const float* drop_masks, float* d_x,
                                      void* stream);
DMME_API int dmme_unet_plan_grad_buckets(const dmme_plan* plan, int64_t* offsets, int64_t* numels, int* bucket_of, int cap);
DMME_API int dmme_unet_backward_cond(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t, int t_len,
                                     const int64_t* labels, const float* d_y, void* workspace, void* bwd_workspace, const float* drop_masks,
                                     float* grad_flat, float* d_x, void* stream, dmme_bucket_fn ready, void* user);
DMME_API int dmme_unet_backward_input_cond(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t,
                                           int t_len, const int64_t* labels, const float* d_y, void* workspace, void* bwd_workspace,
                                           const float* drop_masks, float* d_x, void* stream);
/* test / diagnostic: the kernels a backward of this plan launches, as space-separated key=value pairs
 * ("wgrad_group3x3_jobs=..", "colsum_group_jobs=..", "dgrad[conv3x3_ws2_kernel<11>]=..") */
DMME_API int dmme_unet_plan_bwd_summary(const dmme_plan* plan, char* buf, int cap);
/* diagnostic (tools/l2_stream.py): `blocks` workgroups of 256 threads each stream the same `bytes` (a multiple of 64 KiB) `iters`
 * times with `depth` (1, 2, 4, 8, 16) 16-byte loads in flight per thread; mode 0 loads into registers, mode 1 uses the global -> LDS DMA,
 * mode m >= 2 the DMA in the convolutions' access shape (a wave instruction gathers eight 128-byte rows m 16-byte vectors apart, e.g.
 * 288 = a 3x3 filter row of 256 input channels).  sink: `blocks` uint32 of scratch.  Measures what a CU can draw from L2. */
/* diagnostic (tools/mfma_valu.py): do the MFMAs of one wave and the VALU work of another wave on the same SIMD overlap?  `blocks`
 * workgroups of 512 threads; mode bit 0: MFMA waves run, bit 1: VALU waves run, bit 2: MFMA accumulators in AccVGPRs.  sink: `blocks` floats. */
/* diagnostic (tools/stamp_lvl.py): workgroup `workgroup` of level run `run` writes 100 MHz wall-clock stamps per op iteration into
 * buf ([120][8] int64; NULL: off): 0 start, 1 hand-off seen, 2 input gathered + first filter unit landed, 3 main loop done,
 * 4 epilogue done, 5 stores acknowledged + barrier, 6 flag stored and the next filter stream started. */
DMME_API int dmme_debug_level_stamps(void* buf, int run, int workgroup);
DMME_API int dmme_debug_mfma_valu(int mode, int iters, int blocks, void* sink, void* stream);
/* diagnostic (tools/issue_probe.py): what `n_inner` vector instructions of ONE kind per MFMA slot, issued by the partner wave of an
 * MFMA wave on the same SIMD, cost either wave - all inline asm, per-wave cycle counts (s_memtime) into sink[2 b] (MFMA wave 0) and
 * sink[2 b + 1] (vector wave 4), `blocks` x 2 int64.  kind: 0 v_fma_f32, 1 v_pk_fma_f32, 2 v_exp_f32, 3 v_cvt_pk_bf16_f32,
 * 4 v_pk_mul_f32, 5 v_pk_add_f32, 6 v_add_f32, 7 v_rcp_f32, 8 / 9 the GroupNorm + SiLU prologue of one halo dword in plain / packed
 * instructions, 10 ds_write_b128, 11 ds_read_b128, 12 bf16 unpack (shift / mask), 13 / 14 a 1-KB request in a filter tap's access shape
 * (eight 128-byte rows 2304 bytes apart out of `src`, >= 1.2 MB, L2-resident) by LDS-DMA / into registers, eight in flight per wave.
 * flags: bit 0 MFMA waves run, bit 1 vector waves run, bit 2 / 3 s_setprio 3 on the MFMA / vector waves, bit 4 16x16x32 instead of
 * 32x32x16 MFMAs, bit 5 the MFMA waves also read six 16-byte LDS fragments per eight MFMAs. */
DMME_API int dmme_debug_issue_probe(int kind, int n_inner, int iters, int flags, int blocks, void* sink, const void* src, void* stream);
DMME_API int dmme_debug_l2_stream(const void* buf, int64_t bytes, int iters, int mode, int depth, int blocks, void* sink, void* stream);
/* global L2 norm of a flat fp32 gradient buffer (clip_grad_norm_; scratch: 1024 floats) */
DMME_API int dmme_grad_norm(const float* grad, int64_t numel, float* norm_out, float* scratch, void* stream);
/* one fused pass: clip by global norm (max_norm <= 0: off) -> Adam (torch.optim.Adam, no weight
 * decay; reference lit_modules/ddpm.py:130) -> optional EMA (reference callbacks/ema.py:169-176;
 * ema may be NULL).  `step` is 1-based; grad_norm is the device scalar of dmme_grad_norm.
 * grad_scale multiplies the gradient (and its norm) first: 1 / world when the exchange left rank SUMS in the buffer, else 1. */
DMME_API int dmme_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel,
                            float lr, float beta1, float beta2, float eps, int step, const float* grad_norm, float max_norm,
                            float ema_decay, float grad_scale, void* stream);
/* Dynamic loss scaling for half-precision training (precision="fp16"), device-resident - what torch.cuda.amp.GradScaler does around
 * the reference's `precision: 16`, `amp_backend: native` step (configs/ddpm/cifar10.yaml:53,66; scripts/main.py:44), without a
 * read-back.  amp_state: 8 floats in device memory - [0] scale S, [1] finite steps since the last change of S, [2] optimiser steps
 * taken, [3] found_inf of the last step, [4] steps skipped.
 *   dmme_amp_init:  S = init_scale (GradScaler: 65536), the rest 0.
 *   dmme_amp_scale: grad *= S - on the loss gradient handed to dmme_unet_backward, i.e. backward of S * loss.
 *   dmme_adam_step_amp: dmme_adam_step on the SCALED gradient: divides S out (with grad_scale), clips the unscaled norm (grad_norm is
 *     dmme_grad_norm of the scaled buffer - always required here: it is also the inf / NaN detector), takes the bias-correction step
 *     count from amp_state[2]; a non-finite norm leaves parameters, moments and EMA untouched and multiplies S by backoff_factor
 *     (0.5), growth_interval (2000) finite steps in a row multiply it by growth_factor (2).  Like dmme_adam_step it refuses
 *     numel <= 0 and grad_scale <= 0 (DMME_ERR_INVALID) before anything is launched. */
DMME_API int dmme_amp_init(float* amp_state, float init_scale, void* stream);
DMME_API int dmme_amp_scale(float* grad, int64_t numel, const float* amp_state, void* stream);
DMME_API int dmme_adam_step_amp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, float lr, float beta1,
                                float beta2, float eps, const float* grad_norm, float max_grad_norm, float ema_decay, float grad_scale,
                                float* amp_state, float growth_factor, float backoff_factor, int growth_interval, void* stream);
/* ---- data-parallel gradient exchange with bf16 on the wire (the reference relies on Lightning DDP for this step:
 * configs/ddpm/cifar10.yaml:28,51,62 `devices`, `strategy`, `replace_sampler_ddp`; NCCL's fp32 ring all-reduce there).  One bucket =
 * pack (fp32 -> bf16, zero padded to world * per_rank) -> all-to-all of the per-rank shards (torch.distributed / RCCL) ->
 * shard_reduce (fp32 accumulation in rank order, x scale = 1 / world, ONE rounding) -> all-gather of the bf16 means -> unpack into
 * the fp32 gradient buffer: every rank ends with identical bits; each GPU sends and receives 2 x numel / world x 2 bytes per peer. */
DMME_API int dmme_grad_pack_bf16(const float* grad, int64_t numel, void* dst_bf16, int64_t numel_padded, void* stream);
DMME_API int dmme_shard_reduce_bf16(const void* recv_bf16, int world, int64_t per_rank, float scale, void* out_bf16, void* stream);
DMME_API int dmme_grad_unpack_bf16(const void* src_bf16, int64_t numel, float* grad, void* stream);

/* Copy an intermediate activation (the output of module `name`, e.g. "down_layers.3",
 * "input_conv", "condition") out of the workspace as fp32 NCHW for parity tests.
 * numel_cap guards the destination size. */
DMME_API int dmme_unet_debug_read(const dmme_plan* plan, const void* workspace, const char* name, float* dst,
                         int64_t numel_cap, int64_t* numel_out, void* stream);
/* The same for gradients: after dmme_unet_backward, copy dL/d(output of module `name`) out of the backward workspace
 * (bwd_workspace) as fp32 NCHW.  Every name dmme_unet_debug_read takes holds its full gradient then (every consumer's contribution
 * summed: the next block's, the residual branch's, the concat half of the up block that reads it as a skip).  "condition" fails
 * with DMME_ERR_INVALID: the time-MLP backward overwrites d(temb) in place. */
DMME_API int dmme_unet_debug_read_grad(const dmme_plan* plan, const void* bwd_workspace, const char* name, float* dst,
                         int64_t numel_cap, int64_t* numel_out, void* stream);
/* The GroupNorm statistics a forward that a backward may follow (dmme_unet_forward) left in the workspace for it: the {mean, rstd}
 * rows [B][num_groups][2] of the norm `name`, named by its state_dict prefix ("down_layers.3.conv1.0", "<block>.conv2.0" /
 * "<block>.norm", "<block>.attention.norm", "output_conv.0"), whichever kernel produced them (a norm launch, a conv epilogue, the
 * consuming conv's merge of the producers' partials, the level engine).  Unknown names fail with DMME_ERR_INVALID. */
DMME_API int dmme_unet_debug_read_norm_stats(const dmme_plan* plan, const void* workspace, const char* name, float* dst,
                         int64_t numel_cap, int64_t* numel_out, void* stream);

/* ---- the device random stream (dmme_dropout_masks, dmme_randn, the noise of dmme_chain_update) -----------------------
 * Philox4x32-10 (Salmon et al., SC'11).  A draw is a span (seed, offset, numel); the offset counts quads of 4 values.
 *   counter   quad q of the span uses the 64-bit counter offset + q (mod 2^64) as the counter words {lo, hi, 0, 0}
 *   key       the 64-bit seed as the key words {lo, hi}
 *   order     quad q fills elements 4q .. 4q+3 from its output words x0 .. x3; the last quad is cut off at numel (its other
 *             words are discarded), so a span consumes ceil(numel / 4) counters and the next span starts there
 *   uniform   u(x) = ((x >> 8) + 1) / 2^24, on the grid k / 2^24 with k = 1 .. 2^24: u lies in (0, 1], exact in fp32
 *   normals   (z0, z1) = r (cos a, sin a) with r = sqrt(-2 ln u(x0)), a = fp32(2 pi) * u(x1) rounded to fp32; (z2, z3) the
 *             same from (x2, x3).  u >= 2^-24 bounds every value: |z| <= sqrt(48 ln 2) = 5.768
 *   masks     element i is 0 where u(x_i) <= p (fp32 compare), else 1 / (1 - p) in fp32: drop probability floor(p 2^24) / 2^24
 * The Python side takes the seed and the offset (its offset / 4) from torch's CUDA generator and advances it by 4 ceil(numel / 4)
 * per span; mask draws use the key seed ^ 0x5DEECE66D, a key apart from the noise's under the same seed.
 * tests/philox_ref.py restates this contract in numpy; tests/test_gpu_random.py holds the kernels to it. */

/* Dropout2d multipliers from the library's own Philox stream (train mode without
 * injected masks): keep with probability 1-p, value 1/(1-p); dmme_unet_plan_dropmask_numel values of the stream above. */
DMME_API int dmme_dropout_masks(const dmme_plan* plan, uint64_t seed, uint64_t offset, float* masks, void* stream);

/* ---- diffusion process (elementwise; all NCHW fp32) --------------------------------- */

/* standard normal fill from the library's Philox4x32-10 stream: replaces dmme.gaussian
 * (src/dmme/common/noise.py:4-6) / the draw inside Normal.sample().  out[0 .. numel) receives the normals of the span
 * (seed, offset, numel) of the stream above; nothing past numel is written. */
DMME_API int dmme_randn(float* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream);

/* forward noising: replaces forward_process(...).sample() and the target re-derivation
 * of DDPM.training_step (equations/ddpm/ddpm.py:36-41, diffusion_models/ddpm.py:72-79):
 *   mean = sqrt_abar[t_n] x0 ; std = sqrt_1m_abar[t_n] ; x_t = mean + std z ;
 *   target = (x_t - mean)/std   (optional).
 * sqrt_abar / sqrt_1m_abar: device fp32 tables indexed by t holding sqrt(abar_t) and
 * sqrt(1 - abar_t), evaluated on the host with the reference's fp32 torch ops. */
DMME_API int dmme_q_sample(const float* x0, const float* z, const float* sqrt_abar, const float* sqrt_1m_abar,
                  const int64_t* t, int B, int64_t chw, float* x_t, float* target, void* stream);

/* one DDPM reverse update, in place on x: replaces DDPM.sampling_step after the model
 * call (diffusion_models/ddpm.py:99-110, equations/ddpm/ddpm.py:65-71):
 *   mean = inv_sqrt_alpha * (x - eps_coef * eps);  x = add_noise ? mean + sigma * z : mean
 * The three coefficients are the reference's fp32 values 1/sqrt(alpha_t),
 * beta_t/sqrt(1-abar_t), sqrt(beta_t); add_noise = (t != 1). */
DMME_API int dmme_ddpm_step(float* x, const float* eps, const float* z, float inv_sqrt_alpha, float eps_coef,
                   float sigma, int add_noise, int64_t numel, void* stream);

/* one DDIM update as shipped: replaces DDIM.sampling_step after the model call
 * (diffusion_models/ddim.py:73-77, equations/ddim/ddim.py:52-57):
 *   x = sqrt_abar_prev * ((x - sqrt_one_minus_abar * eps) / sqrt_abar_prev). */
DMME_API int dmme_ddim_step(float* x, const float* eps, float sqrt_one_minus_abar, float sqrt_abar_prev, int64_t numel,
                   void* stream);

/* one paper-form DDIM update (Song et al. 2021, eq. 12), in place on x; the eager twin of DMME_CHAIN_GDDIM (below), bit-identical to it:
 *   x = (k0 * x + k1 * eps) + k2 * z      every product and sum rounded to fp32 on its own (no fma)
 * The host folds the schedule into the three scalars in float64 and rounds them to fp32.  With a = abar[tau_i]:
 *   reverse step to p = abar[tau_{i-1}]:  sigma = eta sqrt((1-p)/(1-a)) sqrt(1 - a/p)  (0 where p == 1 or a == 1),
 *                                         k0 = sqrt(p/a), k1 = sqrt(max(1 - p - sigma^2, 0)) - k0 sqrt(1-a), k2 = sigma
 *   encode step to n = abar[tau_{i+1}]:   k0 = sqrt(n/a), k1 = sqrt(1-n) - k0 sqrt(1-a), k2 = 0
 * z is read only where k2 != 0 and may be NULL otherwise.  The DDIM update dmme_ddim_step computes is the reference's collapsed one
 * (x - sqrt(1-abar_tau_i) eps: the term sqrt(1-abar_prev) eps that points back to x_t is missing) and stays as it is. */
DMME_API int dmme_gddim_step(float* x, const float* eps, const float* z, float k0, float k1, float k2, int64_t numel, void* stream);

/* spherical interpolation between B pairs of images (latents) at n weights, xa / xb: (B, chw), w: n device floats, out: (n, B, chw):
 *   theta_b = acos(clamp(<xa_b, xb_b> / (|xa_b| |xb_b|), -1, 1))
 *   out[j][b] = sin((1 - w_j) theta_b) / sin(theta_b) * xa_b + sin(w_j theta_b) / sin(theta_b) * xb_b
 * and out[j][b] = (1 - w_j) xa_b + w_j xb_b where sin(theta_b) < 1e-6 (parallel images, or one of them zero).
 * Two launches: the three sums per image (several blocks per image, partial sums through a per-device buffer the library owns:
 * calls on one device must be ordered, on one stream or by events), then one pass that reads xa and xb once per tile of 64 weights
 * and writes every weight's output.  The buffer is allocated at the first call and whenever it has to grow, which a stream capture
 * does not allow: make one call of the shape outside a capture first.  chw must be a multiple of 4; n > 0; 0 < B <= 65535; out must
 * not alias xa or xb. */
DMME_API int dmme_slerp(const float* xa, const float* xb, const float* w, int n, int B, int64_t chw, float* out, void* stream);

/* simple_loss (equations/ddpm/losses.py:13): loss[0] = mean((target-eps)^2); optional
 * d_eps = 2 (eps - target) / numel * grad_scale.  `scratch` needs 1024 floats. */
DMME_API int dmme_mse_loss(const float* eps, const float* target, int64_t numel, float* loss, float* d_eps,
                  float grad_scale, float* scratch, void* stream);

/* ---- networks that predict x0 or v instead of the noise (csrc/prediction.hip) -----------------------------------------
 * Every sampler update of this library is written for a noise prediction.  A network trained to predict x0, or v = sqrt(abar_t) eps -
 * sqrt(1 - abar_t) x0 (Salimans & Ho 2022), is served by ONE elementwise launch behind its forward that turns the output into the eps
 * prediction it implies; the update kinds, their tables and their entry points are untouched, and an eps network launches nothing new. */
enum { DMME_PRED_EPS = 0, DMME_PRED_X0 = 1, DMME_PRED_V = 2 };

/* in place on model_out (B, chw), x: the x_t the network was evaluated on:
 *   e = (a[t_b] * out) + (b[t_b] * x)      two products and one sum, each rounded to fp32 on its own (no fma)
 * ab: device fp32 table [T+1][2] = {a_t, b_t}, folded by the host in float64 from alpha_bar and rounded once:
 *   DMME_PRED_X0:  a = -sqrt(abar)/sqrt(1 - abar), b = 1/sqrt(1 - abar); row 0 (abar_0 = 1) is (NaN, NaN): nothing steps from index 0
 *   DMME_PRED_V:   a = sqrt(abar),                 b = sqrt(1 - abar)
 * t: int64 in DEVICE memory, t_len = 1 (every image at t[0]: a chain passes the second word of its loop state) or B (image b at t[b]).
 * An image whose t lies outside 0..T comes out NaN; the table is not read there.  16-byte accesses where chw % 4 == 0 and both
 * pointers are 16-byte aligned, element by element otherwise (any chw).  pred == DMME_PRED_EPS is DMME_ERR_INVALID: do not launch. */
DMME_API int dmme_pred_to_eps(int pred, float* model_out, const float* x, const float* ab, int T, const int64_t* t, int t_len, int B,
                              int64_t chw, void* stream);

/* host-only state of a plan: what its network predicts.  With DMME_PRED_X0 / DMME_PRED_V every capturable step over the plan
 * (dmme_chain_step, dmme_cfg_chain_step, dmme_dpmpp_chain_step, dmme_cfg_dpmpp_chain_step, dmme_repaint_chain_step,
 * dmme_ilvr_chain_step, dmme_ddnm_chain_step, dmme_guided_chain_step) launches dmme_pred_to_eps(pred, model_out, x, ab, T, &state.t, 1, plan batch, C*H*W) directly behind the
 * forward - over all 2B images of a classifier-free plan: the mixing weights 1 - s and s sum to one, so the affine map commutes
 * with e_u + s (e_c - e_u) - and in front of the classifier pass and the update.  `ab` stays the caller's and must outlive every launch and
 * every captured graph that holds its address.  A plan is shared by every process that wraps the same network: set the prediction in
 * front of EVERY chain-step call, DMME_PRED_EPS included (ab is ignored and may be NULL then).  DMME_ERR_UNSUPPORTED: x0 / v on a plan
 * with more than one output plane (an IDDPM network's (eps, v)) or on a classifier; DMME_ERR_INVALID: C*H*W no multiple of 4. */
DMME_API int dmme_unet_plan_set_prediction(dmme_plan* plan, int pred, const float* ab, int T);

/* ---- x0 thresholding in front of every sampler update (csrc/threshold.hip) ---------------------------------------------
 * Every update runs on an eps prediction; the image it implies is x0 = (x_t - sqrt(1 - abar_t) eps) / sqrt(abar_t).  This stage
 * rewrites the eps prediction in place, behind the x0 / v adapter and in front of the update, so that the implied x0 is clipped: the
 * static clip to [-1, 1] (clip_denoised of the published DDPM / IDDPM / ADM samplers) or the dynamic percentile clip of Saharia et al.
 * 2022 (section 2.3).  The update kinds, their tables and their entry points are untouched; with the mode off nothing is launched. */
enum { DMME_THRESHOLD_NONE = 0, DMME_THRESHOLD_STATIC = 1, DMME_THRESHOLD_DYNAMIC = 2 };

/* Per image b at timestep t_b, with table: device fp32 [T+1][4] = {A, B, C, D}_t folded by the host in float64 from alpha_bar and rounded
 * once, A = 1/sqrt(abar), B = sqrt(1 - abar)/sqrt(abar), C = 1/sqrt(1 - abar), D = sqrt(abar)/sqrt(1 - abar); row 0 (abar_0 = 1) is NaN.
 * Every product, difference and quotient is rounded to fp32 on its own (no fma):
 *   x0  = (A x) - (B e)                           e: the eps the update will use
 *   s   = 1                                       static
 *       = max(1, a_k + frac (a_{k+1} - a_k))      dynamic: a_j the j-th smallest (0-based) of the image's chw values |x0|, exact; the host
 *                                                 passes k = floor(p (chw - 1)) and frac = fp32 of the remainder for the percentile p;
 *                                                 a_{k+1} is not looked at where frac == 0 (p = 1: k = chw - 1, frac = 0)
 *   an element with s == 1 and |x0| <= 1 is not stored to: a step that clips nothing leaves the prediction's bits alone
 *   every other element:  e' = (C x) - (D (clamp(x0, -s, s) / s))
 * Non-finite x0: dynamic mode writes NaN to the image's whole eps plane (there is no percentile to take); static mode, which reduces
 * nothing, writes NaN to that element.  An image whose t lies outside 0..T reads the NaN row's fate without touching the table.
 * model_out: [B][planes][chw] with planes 1, or 2 (an IDDPM network's (eps, v): only the eps plane is read and rewritten).  halves == 2
 * (planes == 1): model_out holds 2B images, B conditional then B unconditional, and e is the update's own mix e_u + s_g (e_c - e_u)
 * (three rounded operations, the same device function); e' goes to BOTH halves, so that the update's mix returns it exactly, and an
 * untouched element stays as it is in both; x is read from its first B images.  halves == 1 ignores guidance_scale.
 * t: int64 in DEVICE memory, t_len = 1 or B, as in dmme_pred_to_eps.  Any chw < 2^31; B <= 65535.
 * Static mode is one elementwise launch (16-byte accesses where chw % 4 == 0 and both pointers are aligned).  Dynamic mode selects by
 * radix (four 8-bit digits of the bit pattern of |x0|, integer atomics only: deterministic): one workgroup per image with the image in
 * LDS where chw <= dmme_x0_threshold_lds_capacity() (one launch), else several workgroups per image and per-digit histograms in
 * `scratch` (dmme_x0_threshold_scratch_bytes; seven launches, the first clears the scratch: it need not be zero on entry; no host
 * synchronisation, capturable).  Both forms give the same bits.  scratch may be NULL where the LDS form runs.
 * DMME_ERR_INVALID: mode not 1 or 2, a null table, (k, frac) that no percentile in [0, 1] gives, planes / halves as above. */
DMME_API int dmme_x0_threshold(int mode, float* model_out, const float* x, const float* table, int T, const int64_t* t, int t_len, int B,
                               int64_t chw, int planes, int halves, float guidance_scale, int k, float frac, void* scratch, void* stream);
DMME_API int64_t dmme_x0_threshold_scratch_bytes(int B, int64_t chw);
DMME_API int dmme_x0_threshold_lds_capacity(void); /* elements of one image the one-workgroup form holds */

/* host-only state of a plan, like dmme_unet_plan_set_prediction: with a mode other than DMME_THRESHOLD_NONE every capturable step over
 * the plan launches dmme_x0_threshold behind the adapter and in front of the classifier pass (guided kinds: where ADM's clip_denoised
 * sits) and the update, at t = &state.t, over the plan's batch (a classifier-free kind: two halves of B = plan batch / 2, the guidance
 * scale read on the device from the step's own table row, coef[row length * state.i + scale column]).  table, scratch stay the caller's
 * and must outlive every launch and captured graph; set it in front of EVERY chain-step call (the plan is shared).  Mode 0 clears it
 * and ignores the rest.  DMME_ERR_INVALID: a classifier plan, a null table, (k, frac) out of range for the plan's C*H*W, no scratch
 * where the streaming form would run. */
DMME_API int dmme_unet_plan_set_threshold(dmme_plan* plan, int mode, const float* table, int T, int k, float frac, void* scratch);

/* dmme_q_sample with the regression target of a parameterisation.  x_t: dmme_q_sample's, the same bits.  target (optional):
 *   DMME_PRED_EPS  (x_t - mean)/std, what dmme_q_sample writes, the same bits
 *   DMME_PRED_X0   x0
 *   DMME_PRED_V    (sqrt_abar[t_n] * z) - (sqrt_1m_abar[t_n] * x0), each operation rounded on its own; z is the injected noise */
DMME_API int dmme_q_sample_pred(int pred, const float* x0, const float* z, const float* sqrt_abar, const float* sqrt_1m_abar, const int64_t* t,
                                int B, int64_t chw, float* x_t, float* target, void* stream);

/* MSE with a weight per timestep (min-SNR-gamma, Hang et al. 2023): out, target (B, chw), t: int64[B], w_table: device fp32 indexed by t
 *   loss[0] = 1/(B chw) sum_b w[t_b] sum_j (out - target)^2
 *   d_out (optional) = (out - target) * g_b,  g_b = 2 w[t_b] grad_scale / (B chw) formed once per image and rounded once
 * grad_scale as in dmme_mse_loss (the fp16 loss-scaling path).  Reduced like dmme_mse_loss, with up to 64 blocks per image:
 * `scratch` needs 64 * B floats.  B <= 65535.  The caller guarantees that every t indexes the table. */
DMME_API int dmme_mse_loss_rows(const float* out, const float* target, const float* w_table, const int64_t* t, int B, int64_t chw, float* loss,
                                float* d_out, float grad_scale, float* scratch, void* stream);

/* ---- input pipeline: training batch from an HBM-resident uint8 image set ---------------------------------------------
 * Replaces the per-sample transform chain of the reference's data module (data_modules/cifar10.py:39-44:
 * [RandomHorizontalFlip] -> torchvision ToTensor (uint8 / 255) -> norm, common/norm.py:4-6) plus the DataLoader's collate:
 *   out[b] = (flip[b] ? hflip : id)(data[idx[b]]) / 255, then (x - 0.5) * 2, fp32 NCHW.
 * data: [n_images][C][H][W] uint8 (the CIFAR10 python-pickle layout); idx: int64[B] (caller guarantees 0 <= idx < n_images);
 * flip: uint8[B] or NULL (no augmentation, the reference's test set); W must be a multiple of 4. */
DMME_API int dmme_image_batch(const uint8_t* data, int64_t n_images, const int64_t* idx, const uint8_t* flip, int B, int C, int H, int W,
                     float* out, void* stream);

/* ---- output side: an image batch into the cells of a grid canvas -----------------------------------------------------
 * What the reference's GenerateImage callback does on the host per kept frame (callbacks/generate.py:80: denorm(x_t.clone()))
 * and torchvision's make_grid(padding = pad, pad_value = 0) does once at the end (common/vis.py:25-28), as one launch per frame:
 *   canvas: (Cg, ymaps*(H+pad)+pad, xmaps*(W+pad)+pad), Cg = 3 where C == 1 (the channel is written three times), else C;
 *   image b of x (B, C, H, W; fp32, contiguous) goes to cell k = cell0 + b*cell_stride, at row k / xmaps, column k % xmaps, its
 *   top-left pixel at (row*(H+pad)+pad, col*(W+pad)+pad).
 * value: raw = 0: v = clip((x + 1) / 2, 0, 1), the reference's denorm (common/norm.py:9-11); raw = 1: v = x (frames denormed already).
 * out_kind 0: canvas is fp32 and receives v; out_kind 1: canvas is uint8 and receives (uint8) clamp(v*255 + 0.5, 0, 255), truncated
 * (torchvision's save_image).  Every add and multiply is rounded on its own, so both forms equal numpy float32 bit for bit.
 * Only image pixels are written: the padding keeps what the canvas held (zero it once).  Any H, W; pad >= 0 (pad = 0, one cell: a
 * copy).  DMME_ERR_INVALID: a null pointer, a non-positive size, a cell outside 0 .. xmaps*ymaps-1, cell_stride < 1, out_kind or raw
 * outside {0, 1}. */
DMME_API int dmme_grid_tile(const float* x, int B, int C, int H, int W, int cell0, int cell_stride, int xmaps, int ymaps, int pad, int out_kind,
                   int raw, void* canvas, void* stream);

/* ---- one replayable denoising step ---------------------------------------------------------------------
 * The reference's sampling loops run on the host: `for t in range(T, 0, -1)` around `sampling_step`
 * (diffusion_models/ddpm.py:130, ddim.py:96, iddpm.py), `LitDDPM.forward` builds `torch.tensor([t])` - a host-to-device copy -
 * every step (lit_modules/ddpm.py:77; called per step by callbacks/generate.py:82).  Here everything that varies from step to
 * step is device-resident, so ONE launch sequence (time MLP + UNet + noise draw + update + loop-state advance) serves every
 * step and can be captured in a hipGraph and replayed:
 *   state     64 bytes of device memory (eight 64-bit words): int64 i (loop index), int64 t (= t_table[i], what the network is
 *             evaluated at), uint64 Philox offset in quads, uint64 Philox seed, uint32 ticket + pad, the DPM-Solver++ kinds' "history valid" flag
 *             (cleared by dmme_chain_set, read by no other kind), two reserved words.
 *             dmme_chain_set initialises it (a one-thread kernel: the values travel as kernel arguments, no host buffer to
 *             keep alive, and a graph captured once serves any later seed).
 *   t_table   int64[n+1]: DDPM / IDDPM: t_table[i] = i; DDIM: the tau table (diffusion_models/ddim.py:41-53)
 *   step_coef float[n+1][4], per loop index:
 *             DMME_CHAIN_DDPM  {1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), sqrt(beta_t), -}     (equations/ddpm/ddpm.py:65-71)
 *             DMME_CHAIN_DDIM  {sqrt(1-abar_tau_i), sqrt(abar_tau_{i-1}), -, -}              (equations/ddim/ddim.py:52-57)
 *             DMME_CHAIN_IDDPM {1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), log beta_t, log max(beta~_t, 1e-12)}
 *             DMME_CHAIN_GDDIM {k0, k1, k2, -} of dmme_gddim_step: the paper-form DDIM step at loop index i, for any eta.  The index
 *                              only ever runs downwards, so a chain that ENCODES (x_0 -> x_T) gets reversed tables: row and timestep
 *                              at loop index j describe the step tau_{S-j} -> tau_{S-j+1}
 * dmme_chain_update = the sampler update alone (noise drawn in the kernel from Philox(state.seed, state.offset + quad index): the values
 * dmme_randn would produce at the same offset, so a chain equals the eager loop bit for bit); no noise is added at t == 1 but
 * the offset advances all the same (the reference draws and discards, diffusion_models/ddpm.py:107-110).  After the update the
 * state moves on: i -= 1, t = t_table[i], offset += B*chw/4.  dmme_chain_step = dmme_unet_forward at t = state.t followed by
 * dmme_chain_update; x is updated in place, model_out receives the network output.  chw must be a multiple of 4.
 * DMME_CHAIN_GDDIM draws its normals only at loop indices whose k2 != 0; the offset advances at every step all the same.
 * dmme_chain_update_gddim = dmme_chain_update(DMME_CHAIN_GDDIM, ...) with `noise` (nullable) used in place of the drawn normals (tests). */
enum { DMME_CHAIN_DDPM = 0, DMME_CHAIN_DDIM = 1, DMME_CHAIN_IDDPM = 2, DMME_CHAIN_DDPM_GUIDED = 3, DMME_CHAIN_DDIM_GUIDED = 4, DMME_CHAIN_GDDIM = 5,
       DMME_CHAIN_DDPM_CFG = 6, DMME_CHAIN_GDDIM_CFG = 7 /* classifier-free guidance, below */ };
DMME_API int dmme_chain_set(void* state, int64_t i, const int64_t* t_table, uint64_t philox_seed, uint64_t philox_offset, void* stream);
DMME_API int dmme_chain_update(int kind, float* x, const float* model_out, const float* step_coef, const int64_t* t_table, void* state,
                      int B, int64_t chw, void* stream);
DMME_API int dmme_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, int kind,
                    const float* step_coef, const int64_t* t_table, void* state, void* stream);
DMME_API int dmme_chain_update_gddim(float* x, const float* model_out, const float* noise, const float* step_coef, const int64_t* t_table,
                            void* state, int B, int64_t chw, void* stream);

/* ---- classifier guidance (Dhariwal & Nichol 2021, Algorithms 1 and 2; the reference's src/dmme/guidance/classifier.py sketch) ----
 * dmme_log_softmax_grad: row-wise log-softmax of logits (B, K) fp32 against int64 labels y[B].
 *   mode 0 (training): loss[0] = mean_i -log p(y_i | x_i); d_logits = scale * (softmax_i - onehot(y_i)) / B
 *   mode 1 (guidance): loss[0] = sum_i log p(y_i | x_i);   d_logits = scale * (onehot(y_i) - softmax_i), the gradient of
 *                      scale * sum_i log p(y_i | x_i, t), row by row (no label of one image reaches another's row).
 *   loss / d_logits nullable.  A label outside [0, K) is never used as an index: its row and loss[0] become NaN and *status
 *   (nullable, device int) is set to 1 (the host reads it when it can synchronise; the argument check cannot see device labels).
 * dmme_chain_update_guided: the chain update of DMME_CHAIN_DDPM_GUIDED / DMME_CHAIN_DDIM_GUIDED with grad = d log p(y | x_t, t) / d x_t:
 *   DDPM_GUIDED step_coef {1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), sqrt(beta_t), s*beta_t}:
 *               x = mean + s*beta_t*grad (+ sqrt(beta_t) z, not at t == 1: the mean shift stays)
 *   DDIM_GUIDED step_coef {sqrt(1-abar_tau_i), sqrt(abar_tau_{i-1}), s*sqrt(1-abar_tau_i), -}:
 *               eps' = eps - s*sqrt(1-abar_tau_i)*grad, then the DDIM update with eps'
 *   The Philox stream is consumed exactly as by the unguided kinds; noise (nullable) replaces the drawn normals (tests).
 * dmme_guided_chain_step: one capturable guided step: the UNet's no-grad forward at t = state.t -> model_out; the classifier's
 *   forward (the form a backward follows) at the same device-resident t -> logits; dmme_log_softmax_grad mode 1 (scale 1) against
 *   y -> d_logits; dmme_unet_backward_input -> grad; dmme_chain_update_guided.  Both plans have the same B, H, W; cls is a
 *   DMME_ARCH_CLASSIFIER plan, kind DMME_CHAIN_DDPM_GUIDED or DMME_CHAIN_DDIM_GUIDED.  status: as above (nullable). */
DMME_API int dmme_log_softmax_grad(const float* logits, const int64_t* y, int B, int K, int mode, float scale, float* loss, float* d_logits,
                                   int* status, void* stream);
DMME_API int dmme_chain_update_guided(int kind, float* x, const float* model_out, const float* grad, const float* noise, const float* step_coef,
                                      const int64_t* t_table, void* state, int B, int64_t chw, void* stream);
DMME_API int dmme_guided_chain_step(const dmme_plan* plan, const void* packed, const dmme_plan* cls, const void* cls_packed,
                                    const void* cls_packed_bwd, float* x, float* model_out, void* workspace, void* cls_workspace,
                                    void* cls_bwd_workspace, const int64_t* y, float* logits, float* d_logits, float* grad, int* status,
                                    int kind, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- classifier-free guidance (Ho & Salimans 2021) ------------------------------------------------------------------
 * One network, evaluated with the label and with the null label, replaces the classifier.  Both evaluations ride in ONE forward at batch
 * 2B: x and model_out hold 2B images, the conditional half [0, B) then the unconditional half [B, 2B); labels_2B = (y, K ... K).
 * DMME_CHAIN_DDPM_CFG / DMME_CHAIN_GDDIM_CFG: for element j of image b < B
 *     e^ = e_u + s (e_c - e_u)        three separately rounded fp32 operations (no fma), s = step_coef[i][3]
 *     x' = the DMME_CHAIN_DDPM / DMME_CHAIN_GDDIM update of x[b] with e^ (step_coef[i][0..2] as for the base kind)
 * and x' is stored into both halves of x (which therefore stay equal; x is read from the first).  s = 1 is plain conditional sampling,
 * s = 0 unconditional; Ho & Salimans' w is s - 1.  Column 3 is free in both base kinds, so a table may carry a per-step schedule of s.
 * Noise is indexed by the element of the FIRST half and the offset advances by B*chw/4 per step: a guided chain at batch B consumes
 * exactly the normals of an unguided chain at batch B under the same seed.  B and chw below are those of ONE half.
 * dmme_cfg_step: the eager twin (host scalars; z: B*chw normals, read where the step adds noise - DDPM: add_noise, GDDIM: c2 != 0).
 * dmme_chain_update_cfg: the chain form (device state); noise (nullable) replaces the drawn normals (tests).
 * dmme_cfg_chain_step: one capturable step: dmme_unet_forward_cond (no-grad form) of a DMME_ARCH_DDPM_COND plan of batch 2B at
 *   t = state.t with labels_2B, then dmme_chain_update_cfg at B = plan batch / 2.  status: as dmme_unet_forward_cond (nullable).
 * dmme_label_dropout: the label side of classifier-free training: out[b] = K where u_b < p (and everywhere when p >= 1), else labels[b];
 *   u_b is uniform b of the span (seed, offset, B) of the device random stream above (word b % 4 of quad b / 4, u = ((x >> 8) + 1) / 2^24),
 *   tests/philox_ref.py: uniforms(seed, offset, B).  A label outside [0, K] is copied through and sets *status (nullable, device int).
 *   out must not alias labels. */
DMME_API int dmme_label_dropout(const int64_t* labels, int B, int K, float p, uint64_t seed, uint64_t offset, int64_t* out, int* status, void* stream);
DMME_API int dmme_cfg_step(int kind, float* x, const float* model_out, const float* z, float c0, float c1, float c2, float s, int add_noise, int B,
                           int64_t chw, void* stream);
DMME_API int dmme_chain_update_cfg(int kind, float* x, const float* model_out, const float* noise, const float* step_coef, const int64_t* t_table,
                                   void* state, int B, int64_t chw, void* stream);
DMME_API int dmme_cfg_chain_step(const dmme_plan* plan_2B, const void* packed, float* x_2B, const int64_t* labels_2B, float* model_out, void* workspace,
                                 int* status, int kind, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- DPM-Solver++(2M) (Lu et al. 2022): the second-order multistep solver of the diffusion ODE in data-prediction form -----------
 * alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log(alpha_t / sigma_t); grid tau_0 = 0 < tau_1 < ... < tau_n.  The step from
 * loop index i (a = tau_i) to i - 1 (p = tau_{i-1}), h = lambda_p - lambda_a, with the scalars folded on the host in float64 and rounded to fp32:
 *     x0 = q0 x + q1 e             q0 = 1/alpha_a, q1 = -sigma_a/alpha_a; clamped to [-1, 1] iff clip != 0
 *     D  = history valid ? x0 + w (x0 - x0_prev) : x0        w = h / (2 h_prev), h_prev = lambda_a - lambda_{tau_{i+1}};
 *                                                            w = 0 at i = n, at order 1 and at i = 1
 *     x' = k0 x + k1 D             k0 = sigma_p/sigma_a, k1 = -alpha_p expm1(-h); at i = 1 (p = 0): k0 = 0, k1 = 1 (the chain ends on x0)
 *     history <- x0
 * every product and sum rounded to fp32 on its own (no fma).  Kinds DMME_CHAIN_DPMPP = 8 and DMME_CHAIN_DPMPP_CFG = 9 have entry points and a
 * table layout of their own (dmme_chain_step / dmme_chain_update / dmme_cfg_chain_step refuse them):
 *   step_coef float[n+1][8], per loop index: {q0, q1, k0, k1, w, clip, s, -}    (s: the guidance scale, read by the CFG kind only)
 *   history   fp32, B * chw values in x's layout: the previous step's x0, read and rewritten in place by the thread that owns the quad.  It
 *             is NOT read while the history is not valid, so it needs no initialisation.
 *   state     the loop state of dmme_chain_set; its sixth word is the "history valid" flag: dmme_chain_set clears it (a chain's first
 *             step is first order wherever it starts), the chain forms set it as they advance the state (i -= 1, t = t_table[i]; the Philox
 *             offset stays: the solver draws nothing).
 *   out_planes  chw-sized planes per image of model_out: 1 (eps), or 2 (an IDDPM network's (eps, v): the eps plane is used).
 * dmme_dpmpp_step: the eager twin (row: the 8 floats of one table row in HOST memory; history_valid as an argument), bit-identical to
 * dmme_chain_update_dpmpp, the chain form (row and flag from device memory).  dmme_dpmpp_chain_step = dmme_unet_forward (no-grad form) at
 * t = state.t + dmme_chain_update_dpmpp; a DMME_ARCH_DDPM or DMME_ARCH_IDDPM plan.  The CFG forms: x_2B / model_out hold 2B images
 * (conditional half, unconditional half), e = e_u + s (e_c - e_u) as DMME_CHAIN_GDDIM_CFG forms it, x' goes to both halves, history holds
 * B images; B and chw are those of ONE half.  dmme_cfg_dpmpp_chain_step: a DMME_ARCH_DDPM_COND plan of batch 2B; status as
 * dmme_unet_forward_cond (nullable).  chw must be a multiple of 4. */
enum { DMME_CHAIN_DPMPP = 8, DMME_CHAIN_DPMPP_CFG = 9 };
DMME_API int dmme_dpmpp_step(float* x, const float* model_out, float* history, const float* row, int history_valid, int B, int64_t chw, int out_planes,
                             void* stream);
DMME_API int dmme_chain_update_dpmpp(float* x, const float* model_out, float* history, const float* step_coef, const int64_t* t_table, void* state, int B,
                                     int64_t chw, int out_planes, void* stream);
DMME_API int dmme_dpmpp_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, float* history,
                                   const float* step_coef, const int64_t* t_table, void* state, void* stream);
DMME_API int dmme_cfg_dpmpp_step(float* x_2B, const float* model_out, float* history, const float* row, int history_valid, int B, int64_t chw, void* stream);
DMME_API int dmme_chain_update_cfg_dpmpp(float* x_2B, const float* model_out, float* history, const float* step_coef, const int64_t* t_table, void* state,
                                         int B, int64_t chw, void* stream);
DMME_API int dmme_cfg_dpmpp_chain_step(const dmme_plan* plan_2B, const void* packed, float* x_2B, const int64_t* labels_2B, float* model_out, void* workspace,
                                       int* status, float* history, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- RePaint inpainting (Lugmayr et al. 2022) and SDEdit image editing (Meng et al. 2022): conditioning an unconditional network on pixels ----
 * Grid 0 = tau_0 < tau_1 < ... < tau_n = T; a level k is a sample at noise level tau_k.  RePaint walks the levels n -> 0 with jumps back
 * up; every downward transition a -> b = a - 1 is one network evaluation and one table row.  The upward transitions that follow it (b -> c,
 * c = b or b + jump length) use no network and forward noising composes, so the row carries them FOLDED into one Gaussian,
 *     q(x_c | x_b) = N(sqrt(abar_c / abar_b) x_b, (1 - abar_c / abar_b) I)         (abar at tau_c, tau_b)
 * which has the distribution of the single sqrt(1 - beta) x + sqrt(beta) z steps it replaces, not their draws.  A plain walk n -> 0 (no
 * jump in any row) is the SDEdit chain.  Kind DMME_CHAIN_REPAINT = 10 has entry points and a table layout of its own (dmme_chain_step and
 * dmme_chain_update refuse it):
 *   step_coef float[n_rows+1][8], per loop index (i runs n_rows .. 1, one row per downward transition; alpha = abar_a / abar_b, beta = 1 - alpha):
 *             {c0 = 1/sqrt(alpha), c1 = beta/sqrt(1 - abar_a), c2 = sqrt(beta) (0 where b = 0), ka = sqrt(abar_b), ks = sqrt(1 - abar_b),
 *              r0 = sqrt(abar_c / abar_b), r1 = sqrt(1 - abar_c / abar_b) (exactly 1, 0 where c = b), -}
 *   t_table   int64[n_rows+1]: t_table[i] = tau_a, what the network is evaluated at; t_table[0] = 0
 *   known, mask   fp32, B * chw values each in x's layout, read only: the image whose pixels are kept and m in [0, 1] (1: known, 0: generate)
 *   the update, every product, sum and difference rounded to fp32 on its own (no fma):
 *     u  = c0 (x - c1 e);      u = u + c2 z0          only where c2 != 0        the reverse step of the unknown pixels
 *     k  = ka x0;              k = k + ks z1          only where ks != 0        the known pixels at level b
 *     y  = m k + (1 - m) u
 *     x' = y;                  x' = r0 y + r1 z2      only where r1 != 0        the folded jump b -> c
 *   normals   a step owns THREE streams of B*chw normals: stream s of quad q is the draw at Philox counter offset + s * (B*chw/4) + q, so
 *             dmme_randn(z3, 3*B*chw, seed, offset) writes exactly the [3][B*chw] block the eager form reads.  Which streams a step uses is
 *             decided by its row (c2, ks, r1), not by t; a stream whose coefficient is zero is neither drawn nor read.  The chain form moves
 *             the offset by 3 * B*chw/4 per step whatever the row used.
 *   out_planes  as for DPM-Solver++: 1 (eps), or 2 (an IDDPM network's (eps, v): the eps plane is used).
 * dmme_repaint_step: the eager twin (row: 8 floats in HOST memory; z3: the [3][B*chw] block, nullable only where the row uses no stream),
 * bit-identical to dmme_chain_update_repaint, the chain form (row from device memory, normals drawn in the kernel; noise: nullable, a
 * [3][B*chw] block used in place of the drawn normals - tests).  dmme_repaint_chain_step = dmme_unet_forward (no-grad form) at t = state.t +
 * dmme_chain_update_repaint; an unconditional DMME_ARCH_DDPM or DMME_ARCH_IDDPM plan.  chw must be a multiple of 4. */
enum { DMME_CHAIN_REPAINT = 10 };
DMME_API int dmme_repaint_step(float* x, const float* model_out, const float* known, const float* mask, const float* z3, const float* row, int B,
                               int64_t chw, int out_planes, void* stream);
DMME_API int dmme_chain_update_repaint(float* x, const float* model_out, const float* known, const float* mask, const float* noise,
                                       const float* step_coef, const int64_t* t_table, void* state, int B, int64_t chw, int out_planes, void* stream);
DMME_API int dmme_repaint_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, const float* known,
                                     const float* mask, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- ILVR (Choi et al. 2021): sampling that shares the coarse content of a reference image (csrc/ilvr.hip) ----------------------------
 * Grid and levels as RePaint's; the walk goes straight down, n -> 0, one network evaluation and one table row per transition
 * a -> b = a - 1.  With y the clean reference and phi a linear low-pass filter, a step is DDPM's reverse step followed by the
 * refinement x' = phi(y_b) + u - phi(u) of the paper, written with ONE filter application because phi is linear:
 *     u  = c0 (x - c1 e);      u = u + c2 z0          only where c2 != 0        DDPM's reverse step (sigma^2 = beta), DDPM's bits
 *     if g != 0:
 *         k  = ka y;           k = k + ks z1          only where ks != 0        the reference noised to level b
 *         d  = k - u
 *         x' = u + phi(d)                              phi(d) = Ph d Pw^T per channel plane of H x W
 *     else x' = u
 * Kind DMME_CHAIN_ILVR = 11 has entry points and a table layout of its own and no row in the kind table of the elementwise updates:
 * dmme_chain_step and dmme_chain_update refuse it.
 *   step_coef float[n+1][8], per loop index (alpha = abar_a / abar_b):
 *             {c0 = 1/sqrt(alpha), c1 = (1 - alpha)/sqrt(1 - abar_a), c2 = sqrt(1 - alpha) (0 where b = 0), ka = sqrt(abar_b),
 *              ks = sqrt(1 - abar_b) (0 at b = 0), g = 1 while the step is conditioned else 0, -, -}
 *   t_table   int64[n+1]: t_table[i] = tau_a; t_table[0] = 0
 *   ref       fp32, B * chw values in x's layout, read only
 *   Ph, Pw    device fp32, [H][H] and [W][W] row-major: per axis of length n the product R(n/N -> n) R(n -> n/N) of the two bicubic
 *             (a = -0.5) resize matrices, antialiased on the way down, windows clipped to the image and renormalised (rows sum to 1),
 *             which the host builds in float64 and rounds once.  The library reads them as dense matrices and assumes nothing else.
 *   rounding  the elementwise half rounds every product, sum and difference to fp32 on its own (no fma), so with g = 0 the step is
 *             dmme_ddpm_step bit for bit.  The filter is T = d Pw^T, then F = Ph T: each value is the chain
 *             acc = fma(a_k, b_k, acc), k = 0, 1, ... from acc = 0, in ONE device function that every form calls; x' = u + F is one
 *             more rounded sum.  Hence |F - exact| <= (H + W + 8) 2^-24 (|Ph| |d| |Pw|^T) elementwise.
 *   normals   a step owns TWO streams of B*chw normals: stream s of quad q is the draw at Philox counter offset + s * (B*chw/4) + q, so
 *             dmme_randn(z2, 2*B*chw, seed, offset) writes exactly the [2][B*chw] block the eager form reads.  A stream whose
 *             coefficient is zero is neither drawn nor read, and an unconditioned row never touches z1.  The chain form moves the
 *             offset by 2 * B*chw/4 per step whatever the row used.
 *   forms     fused: planes of H*W <= dmme_lowpass_lds_capacity() values whose tables fit beside them (64 x 64 and 32 x 32 do) take ONE
 *             launch, one workgroup per plane: d, T and both tables in LDS, u in registers, x' stored 16 bytes at a time; in place is
 *             safe because a plane is read completely before it is written.  Streaming: larger planes (256 x 256; H <= 384,
 *             W <= 767) take two launches, a row pass that writes T to `scratch` (dmme_lowpass_scratch_bytes(B*C, H, W) bytes) and a
 *             column pass that recomputes u from the same operands and Philox counters; the loop state advances at the end of the
 *             second.  force_streaming != 0 sends a plane that fits the fused form through the streaming one: the same bits.
 *   out_planes  1 (eps), or 2 (an IDDPM network's (eps, v): the eps plane is used).
 * C*H*W and W must be multiples of 4.  dmme_lowpass applies phi alone to `planes` planes (dst may equal src).  dmme_ilvr_step: the eager
 * twin (row: 8 floats in HOST memory; z2: the [2][B*chw] block, nullable only where the row uses no stream), bit-identical to
 * dmme_chain_update_ilvr, the chain form (row from device memory at step_coef[8 i], normals drawn in the kernel; noise: nullable, a
 * [2][B*chw] block used in place of the drawn normals - tests).  dmme_ilvr_chain_step = dmme_unet_forward (no-grad form) at t = state.t,
 * the x0 / v adapter and x0 thresholding as every chain step has them, then dmme_chain_update_ilvr; an unconditional DMME_ARCH_DDPM or
 * DMME_ARCH_IDDPM plan. */
enum { DMME_CHAIN_ILVR = 11 };
DMME_API int dmme_lowpass(const float* src, float* dst, int planes, int H, int W, const float* Ph, const float* Pw, float* scratch, int force_streaming,
                          void* stream);
DMME_API int dmme_lowpass_lds_capacity(void);
DMME_API int64_t dmme_lowpass_scratch_bytes(int planes, int H, int W);
DMME_API int dmme_ilvr_step(float* x, const float* model_out, const float* ref, const float* z2, const float* row, const float* Ph, const float* Pw,
                            float* scratch, int B, int C, int H, int W, int out_planes, int force_streaming, void* stream);
DMME_API int dmme_chain_update_ilvr(float* x, const float* model_out, const float* ref, const float* noise, const float* Ph, const float* Pw, float* scratch,
                                    const float* step_coef, const int64_t* t_table, void* state, int B, int C, int H, int W, int out_planes,
                                    int force_streaming, void* stream);
DMME_API int dmme_ilvr_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, const float* ref, const float* Ph,
                                  const float* Pw, float* scratch, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- DDNM (Wang, Yu, Zhang 2023): zero-shot restoration from a measurement y = A x (csrc/ddnm.hip) ------------------------------------
 * The operator family is A = M o Pool_s o Gray_g on images (B, C, H, W): Gray_g the mean over the C channels where gray = 1 (Cm = 1),
 * the identity where gray = 0 (Cm = C); Pool_s the mean over s x s blocks, to (B, Cm, h, w) = (B, Cm, H/s, W/s), s >= 1 a divisor of H
 * and W; M a binary mask at measurement resolution, 1 = measured.  A cell is the n = (C if gray else 1) s s image elements one
 * measurement value averages; the pseudo-inverse A+ y gives every element of a cell the value m y of the cell (A A+ A = A holds for a
 * binary mask only).  Grid and levels as RePaint's, the walk that of repaint_levels ("time travel"); a downward transition
 * a -> b = a - 1 is one network evaluation and one table row (DDNM+, eq. 17-19 of the paper; alpha = abar_a / abar_b, beta = 1 - alpha):
 *     x0 = (A_t x) - (B_t e)                                         rounded like dmme_x0_threshold's x0
 *     r  = mean_cell(x0) - y   where the cell's m != 0, else 0       one value per cell; y is not looked at where m == 0
 *     xh = x0 - lambda r
 *     u  = ca xh;   u = u + cb x   only where cb != 0;   u = u + cz z0   only where cz != 0
 *     x' = u, or (r0 u) + (r1 z1)  only where r1 != 0                the walk's next upward run b -> c folded into one Gaussian, as RePaint's
 * Kind DMME_CHAIN_DDNM = 12 has entry points and a table layout of its own and no row in the kind table of the elementwise updates:
 * dmme_chain_step and dmme_chain_update refuse it.
 *   step_coef float[n_rows+1][8], per loop index, with sigma_y the noise level of the measurement, var = beta (1 - abar_b)/(1 - abar_a):
 *             {ca = sqrt(abar_b) beta/(1 - abar_a), cb = sqrt(alpha) (1 - abar_b)/(1 - abar_a), cz = sqrt(max(var - (ca lambda sigma_y)^2, 0)),
 *              A_t = 1/sqrt(abar_a), B_t = sqrt(1 - abar_a)/sqrt(abar_a), lambda = 1 where sigma_y = 0 or sqrt(var) >= ca sigma_y, else
 *              sqrt(var)/(ca sigma_y), r0 = sqrt(abar_c / abar_b), r1 = sqrt(1 - abar_c / abar_b) (1, 0 where no upward run follows)};
 *             for b = 0 the row is exactly {1, 0, 0, A_t, B_t, lambda, 1, 0}: the last step returns xh bit for bit.  The host builds the
 *             rows in float64 and rounds them once.
 *   t_table   int64[n_rows+1]: t_table[i] = tau_a; t_table[0] = 0
 *   y, mask   fp32, (B, Cm, h, w) contiguous, read only; the mask's values are 0 or 1
 *   rounding  every product, sum and difference is rounded to fp32 on its own (no fma).  A cell's mean is ONE chain: acc = the cell's
 *             first element, acc = acc + next in the order (channel,) row, column, then acc / n correctly rounded - in one device
 *             function that dmme_ddnm_measure and both update forms call.  Hence |mean - exact| <= (n + 1) 2^-24 max|element|, the
 *             same bits from every entry point, whatever B and the image's place in the batch.
 *   normals   a step owns TWO streams of B*chw normals: stream s of the quad at element g is the draw at Philox counter
 *             offset + s * (B*chw/4) + g/4, so dmme_randn(z2, 2*B*chw, seed, offset) writes exactly the [2][B*chw] block the eager form
 *             reads.  A stream whose coefficient (cz, r1) is zero is neither drawn nor read.  The chain form moves the offset by
 *             2 * B*chw/4 per step whatever the row used.
 *   forms     quad (n == 1, plain inpainting): elementwise, no LDS.  Band (every other case): one workgroup per image and band of s rows
 *             across all C channels, x0 staged in LDS, one launch; in place is safe because a band is read completely before it is
 *             written.  A band holds C*s*W values, at most dmme_ddnm_band_capacity() (3 x 32 x 256 fits); a larger one is refused with
 *             DMME_ERR_UNSUPPORTED, as is a band whose staging with one residual per cell exceeds 159 KiB of LDS.
 *   out_planes  1 (eps), or 2 (an IDDPM network's (eps, v): the eps plane is used).
 * W (and with it C*H*W) must be a multiple of 4 (DMME_ERR_UNSUPPORTED otherwise).  dmme_ddnm_measure: y_out = A x (mask nullable: all
 * measured; an unmeasured cell gives 0).  dmme_ddnm_step: the eager twin (row: 8 floats in HOST memory; z2: the [2][B*chw] block,
 * nullable only where the row uses no stream), bit-identical to dmme_chain_update_ddnm, the chain form (row from device memory at
 * step_coef[8 i], normals drawn in the kernel; noise: nullable, a [2][B*chw] block used in place of the drawn normals - tests).
 * dmme_ddnm_chain_step = dmme_unet_forward (no-grad form) at t = state.t, the x0 / v adapter and x0 thresholding as every chain step has
 * them, then dmme_chain_update_ddnm; an unconditional DMME_ARCH_DDPM or DMME_ARCH_IDDPM plan. */
enum { DMME_CHAIN_DDNM = 12 };
DMME_API int dmme_ddnm_band_capacity(void);
DMME_API int dmme_ddnm_measure(const float* x, const float* mask, float* y_out, int B, int C, int H, int W, int s, int gray, void* stream);
DMME_API int dmme_ddnm_step(float* x, const float* model_out, const float* y, const float* mask, const float* z2, const float* row, int B, int C, int H, int W,
                            int s, int gray, int out_planes, void* stream);
DMME_API int dmme_chain_update_ddnm(float* x, const float* model_out, const float* y, const float* mask, const float* noise, const float* step_coef,
                                    const int64_t* t_table, void* state, int B, int C, int H, int W, int s, int gray, int out_planes, void* stream);
DMME_API int dmme_ddnm_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, const float* y, const float* mask,
                                  int s, int gray, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- DPS (Chung et al., ICLR 2023, Algorithm 1): posterior sampling for noisy linear inverse problems (csrc/dps.hip) ------------------
 * The operator family acts on each channel plane of images (B, C, H, W): A x = M o (Kh x_c Kw^T), to (B, C, h, w), with Kh [h][H] and
 * Kw [w][W] dense fp32 row-major device matrices, h <= H, w <= W, and M a binary mask at measurement resolution, 1 = measured.  The
 * library reads the matrices as dense and assumes nothing else (the host builds identity, Gaussian blur, bicubic and average presets in
 * float64 and rounds them once).  Grid and levels as RePaint's; the walk goes straight down, n -> 0, one network evaluation, one input
 * gradient and one table row per transition a -> b = a - 1 (alpha = abar_a / abar_b).  A step is DDPM's reverse step followed by a
 * gradient step on ||y - A x0^(x_t)|| taken through the network:
 *     x0 = (A_t x) - (B_t e)                                          rounded like dmme_x0_threshold's x0
 *     T  = x0 Kw^T;  Y = Kh T                                         per plane
 *     r  = y - Y   where the cell's m != 0, else 0                    a select: y is not looked at where m == 0 (a NaN there stays out)
 *     U  = r Kw;   g = Kh^T U                                         g = A^T r
 *     d_out = B_t g  (the eps plane; an IDDPM output's v plane: 0);   sumsq[b][c] = sum r^2 over the plane
 *     dx = J_eps(x_t)^T d_out                                         dmme_unet_backward_input behind the keep form of the forward
 *     u  = c0 (x - c1 e);      u = u + c2 z   only where c2 != 0      DDPM's reverse step (sigma^2 = 1 - alpha), DDPM's bits
 *     n_b = sqrt(sum_c sumsq[b][c])                                   in channel order; per image
 *     x' = u + (zeta / n_b)((A_t g) - dx)   where zeta != 0 and n_b != 0, else x' = u (g, dx and sumsq are not read where zeta == 0)
 * The sign: grad_{x_t} ||r|| = (-A_t g + J_eps^T (B_t g)) / ||r||.  The backward is linear in d_y and independent per image, so the factor
 * 1 / ||r_b|| is applied in the update and no grid-wide reduction sits between the adjoint kernel and the backward.
 * Kind DMME_CHAIN_DPS = 13 has entry points and a table layout of its own and no row in the kind table of the elementwise updates:
 * dmme_chain_step and dmme_chain_update refuse it.
 *   step_coef float[n+1][8], per loop index: {c0 = 1/sqrt(alpha), c1 = (1 - alpha)/sqrt(1 - abar_a), c2 = sqrt(1 - alpha) (0 where b = 0),
 *             A_t = 1/sqrt(abar_a), B_t = sqrt(1 - abar_a)/sqrt(abar_a), zeta, -, -}; built in float64, rounded once
 *   t_table   int64[n+1]: t_table[i] = tau_a; t_table[0] = 0
 *   y, mask   fp32, (B, C, h, w) contiguous, read only; the mask's values are 0 or 1 (mask nullable: everything is measured)
 *   g, dx     fp32 (B, C, H, W);  d_out: fp32 in the network output's layout (B, out_planes * C, H, W);  sumsq: fp32 [B][C]
 *   rounding  the elementwise parts round every product, sum, difference, quotient and root to fp32 on its own (no fma), so with
 *             zeta = 0 the update is dmme_ddpm_step bit for bit.  Each of the four matrix products is the chain
 *             acc = fma(a_k, b_k, acc), k = 0, 1, ... from acc = 0, in ONE device function that dmme_dps_measure and both adjoint forms
 *             call: |Y - exact| <= (H + W + 8) 2^-24 (|Kh| |x0| |Kw|^T) elementwise, and so on stage by stage.  sumsq is each thread's
 *             cells in ascending order, then a fixed tree over the workgroup's 256 partial sums: no atomics, the same bits every run,
 *             whatever B and the image's place in the batch.
 *   normals   a step owns ONE stream of B*chw normals: the quad at element e is the draw at Philox counter offset + e/4, what
 *             dmme_randn(z, B*chw, seed, offset) writes.  Where c2 == 0 nothing is drawn or read.  The chain form moves the offset by
 *             B*chw/4 per step whatever the row used.
 *   form      one workgroup per (image, channel) plane with the plane, T, r and both tables in LDS
 *             (H W + H w + h w + h (H + 1) + w (W + 1) + 256 floats, at most 96 KiB: 32 x 32 and 64 x 64 with h = H, w = W fit).  A plane
 *             of more than dmme_dps_capacity() values, or one whose tables do not fit beside it, is refused with DMME_ERR_UNSUPPORTED
 *             before any launch; a streaming form is not built.  C*H*W and W must be multiples of 4 (DMME_ERR_UNSUPPORTED).
 *   out_planes  1 (eps), or 2 (an IDDPM network's (eps, v): the eps plane is used, the v plane's gradient is 0).
 * dmme_dps_measure: y_out = A x (an unmeasured cell is exactly 0).  dmme_dps_adjoint: g, d_out and sumsq from (x, model_out) with the row
 * (8 floats) in HOST memory; dmme_chain_adjoint_dps: the same bits with the row read at step_coef[8 state.i] (the state is only read).
 * dmme_dps_step: the eager update (row in HOST memory; z nullable only where c2 == 0; g, dx, sumsq nullable only where zeta == 0),
 * bit-identical to dmme_chain_update_dps, the chain form (row from device memory, normals drawn in the kernel; noise: nullable, B*chw
 * normals used in place of the drawn ones - tests; the last block advances the loop state).
 * dmme_dps_chain_step = dmme_unet_forward (the KEEP form: `packed` holds the unfolded weights) at t = state.t, dmme_chain_adjoint_dps,
 * dmme_unet_backward_input (packed_bwd, bwd_workspace: as there), dmme_chain_update_dps: one keep-forward plus one input-backward per step.
 * An unconditional DMME_ARCH_DDPM or DMME_ARCH_IDDPM plan (DMME_ERR_INVALID otherwise) whose prediction is eps and whose threshold mode
 * is none (DMME_ERR_UNSUPPORTED otherwise: the derivative of the adapter and of the clip is not built). */
enum { DMME_CHAIN_DPS = 13 };
DMME_API int dmme_dps_capacity(void);
DMME_API int dmme_dps_measure(const float* x, const float* Kh, const float* Kw, const float* mask, float* y_out, int B, int C, int H, int W, int h, int w,
                              void* stream);
DMME_API int dmme_dps_adjoint(const float* x, const float* model_out, int out_planes, const float* row, const float* y, const float* mask, const float* Kh,
                              const float* Kw, float* g, float* d_out, float* sumsq, int B, int C, int H, int W, int h, int w, void* stream);
DMME_API int dmme_chain_adjoint_dps(const float* x, const float* model_out, int out_planes, const float* step_coef, const void* state, const float* y,
                                    const float* mask, const float* Kh, const float* Kw, float* g, float* d_out, float* sumsq, int B, int C, int H, int W, int h,
                                    int w, void* stream);
DMME_API int dmme_dps_step(float* x, const float* model_out, const float* g, const float* dx, const float* sumsq, const float* z, const float* row, int B, int C,
                           int H, int W, int out_planes, void* stream);
DMME_API int dmme_chain_update_dps(float* x, const float* model_out, const float* g, const float* dx, const float* sumsq, const float* noise,
                                   const float* step_coef, const int64_t* t_table, void* state, int B, int C, int H, int W, int out_planes, void* stream);
DMME_API int dmme_dps_chain_step(const dmme_plan* plan, const void* packed, const void* packed_bwd, float* x, float* model_out, void* workspace,
                                 void* bwd_workspace, const float* y, const float* mask, const float* Kh, const float* Kw, int h, int w, float* g, float* d_out,
                                 float* dx, float* sumsq, const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- probability-flow ODE (Song et al., ICLR 2021, section 4.3 and appendix D.2): Heun sampler, latent encoding, log-likelihood
 * (csrc/pfode.hip) ---------------------------------------------------------------------------------------------------------------------
 * With sig(t) = sqrt((1 - abar_t) / abar_t) and xbar = x / sqrt(abar) the ODE is d xbar / d sig = eps(x, t), and along a solution
 * d log pbar / d sig = -sqrt(abar) tr(d eps / d x).  The nodes are integer timesteps g_0 < ... < g_n.  A Heun (trapezoid) step a -> b, in
 * either direction, has k0 = sqrt(abar_b / abar_a), k1 = sqrt(1 - abar_b) - k0 sqrt(1 - abar_a), h = sig(b) - sig(a) and two stages:
 *     A (at x_a, t = a):  e_a = eps(x_a, a);  x' = k0 x_a + k1 e_a                       the paper-form DDIM step, eta = 0
 *     B (at x', t = b):   e_b = eps(x', b);   x_b = k0 x_a + (k1 / 2)(e_a + e_b)
 * With the likelihood on, a stage also draws a Rademacher probe z, forms s[img] = sum z (J^T z) with J^T z from dmme_unet_backward_input
 * (d_out = z in the eps plane, 0 in the v plane of a two-plane output) and adds w s to a per-image double: w_A = (h / 2) sqrt(abar_a),
 * w_B = (h / 2) sqrt(abar_b).  Walking up from x_{g_0} := x_0:  log p(x_0) = log N(x_T; 0, I) + (D / 2)(ln abar_{g_n} - ln abar_{g_0}) + acc.
 * Kind DMME_CHAIN_PFODE = 14 has entry points and a table layout of its own: dmme_chain_step and dmme_chain_update refuse it.
 *   step_coef float[n+1][8], per loop index (one STAGE per index, the index runs down): {c0, c1, c2, c3, w, save, 0, 0}, folded by the
 *             host in float64 and rounded once.  A: (k0, 0, k1, 0, w_A, 1); B: (0, k0, k1/2, k1/2, w_B, 0); the closing Euler stage
 *             g_0 -> 0 of a decoding walk: (1/sqrt(abar), 0, -sqrt(1 - abar)/sqrt(abar), 0, 0, 0) at g_0.  Row 0 is never stepped from.
 *   t_table   int64[n+1]: the timestep the network is evaluated at from loop index i
 *   update    THE stage update, one device function (pf_update) that the eager and the chain form both call, in this order:
 *                 r = 0;  r = c0 * x (rounded);  r = fma(c1, xs, r);  r = fma(c2, e, r);  r = fma(c3, es, r);  x_new = r
 *             a term whose coefficient is 0 is skipped and its operand is not read (xs and es may hold anything in front of a stage A).
 *             Where save != 0, xs <- x and es <- e take the values from before the update.  e is the eps plane of model_out
 *             (out_planes 1 or 2).  |x_new - exact| <= 4 * 2^-24 (|c0 x| + |c1 xs| + |c2 e| + |c3 es|).  Quads where chw % 4 == 0 (or
 *             B = 1 with one plane) and every pointer is 16-byte aligned, the last numel % 4 elements one by one; else element by element.
 *   probe     the span contract of the Philox section above holds unchanged: quad q uses counter offset + q and fills elements
 *             4q .. 4q+3 of the B*chw values, the last quad cut off at numel; element i is -1.0f where bit 31 of its word is set, else
 *             +1.0f.  dmme_pf_probe writes it into a buffer of the network output's layout (B, out_planes * chw): the eps plane = z,
 *             the v plane = 0; the dot reads z back from there.  dmme_rademacher(out, numel, ...) is the same launch with one plane.
 *             A likelihood chain moves the offset by B*chw/4 per stage.
 *   dot       s[img] = sum z dx: block (p, img) of a grid (parts, B) sums its share (each thread its elements in ascending order by fma,
 *             the wave by a butterfly, the waves in index order) into scratch[img * parts + p]; parts depends on chw alone.  ONE
 *             finishing launch adds the partials in index order in double, writes s_out[img] = (float)S and does
 *             acc[img] += (double)w * (double)s_out[img] (two roundings).  No atomics, no workgroup waits for another: equal inputs give
 *             equal bits, and an image's value does not depend on its place in a larger batch.
 *             |s - exact| <= (chw + 8) 2^-24 sum |z dx|.  scratch: dmme_pf_scratch_floats(B, chw) floats.
 *   prior     dmme_pf_prior: out[img] = -(1/2) sum x^2 - (chw / 2) ln(2 pi) in double, the same two launches over (x, x).
 *   dequantize  dmme_pf_dequantize: x += (u - 0.5) * fp32(2 / 255) with the contract's u of the span (seed, offset, numel); the difference is
 *             exact, the product and the sum round once each.
 * dmme_pf_stage / dmme_pf_dot take their row (8 floats) from HOST memory; dmme_chain_stage_pf / dmme_chain_dot_pf / dmme_chain_probe_pf
 * read it (and the probe's seed and offset) at the loop state, give the same bits, and only the stage advances the state (i -= 1,
 * t = t_table[i]; the offset by B*chw/4 where advance_offset != 0).
 * dmme_pf_chain_step = the no-grad forward at t = state.t behind the front every chain step has (the x0 / v adapter, x0 thresholding), then
 * dmme_chain_stage_pf: encoding and decoding differ only in their tables.  dmme_pf_ll_chain_step = dmme_unet_forward (the KEEP form:
 * `packed` holds the unfolded weights), dmme_chain_probe_pf, dmme_unet_backward_input, dmme_chain_dot_pf, dmme_chain_stage_pf: one
 * keep-forward plus one input-backward per stage; plans as dmme_dps_chain_step's (unconditional, eps, no threshold).  Both are capturable
 * and never synchronise with the host.
 * dmme_unet_backward_input leaves the forward's saved context intact: it reads the forward's workspace, writes its gradients into
 * bwd_workspace and d_x, and the only part of `workspace` it writes is the split-K scratch of the small-map convolutions, which
 * holds no saved activation (the forward uses it the same way).  A second probe of the same forward would cost one more input-backward and no forward (not built: tile the batch). */
enum { DMME_CHAIN_PFODE = 14 };
DMME_API int dmme_rademacher(float* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream);
DMME_API int dmme_pf_probe(float* d_out, int B, int64_t chw, int out_planes, uint64_t seed, uint64_t offset, void* stream);
DMME_API int dmme_chain_probe_pf(float* d_out, const void* state, int B, int64_t chw, int out_planes, void* stream);
DMME_API int dmme_pf_dequantize(float* x, int64_t numel, uint64_t seed, uint64_t offset, void* stream);
DMME_API int64_t dmme_pf_scratch_floats(int B, int64_t chw);
DMME_API int dmme_pf_dot(const float* d_out, int out_planes, const float* dx, const float* row, int B, int64_t chw, float* scratch, float* s_out, double* acc,
                         void* stream);
DMME_API int dmme_chain_dot_pf(const float* d_out, int out_planes, const float* dx, const float* step_coef, const void* state, int B, int64_t chw,
                               float* scratch, float* s_out, double* acc, void* stream);
DMME_API int dmme_pf_prior(const float* x, int B, int64_t chw, float* scratch, double* out, void* stream);
DMME_API int dmme_pf_stage(float* x, const float* model_out, int out_planes, float* xs, float* es, const float* row, int B, int64_t chw, void* stream);
DMME_API int dmme_chain_stage_pf(float* x, const float* model_out, int out_planes, float* xs, float* es, const float* step_coef, const int64_t* t_table,
                                 void* state, int advance_offset, int B, int64_t chw, void* stream);
DMME_API int dmme_pf_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, float* xs, float* es,
                                const float* step_coef, const int64_t* t_table, void* state, void* stream);
DMME_API int dmme_pf_ll_chain_step(const dmme_plan* plan, const void* packed, const void* packed_bwd, float* x, float* model_out, void* workspace,
                                   void* bwd_workspace, float* xs, float* es, float* d_out, float* dx, float* scratch, float* s_out, double* acc,
                                   const float* step_coef, const int64_t* t_table, void* state, void* stream);

/* ---- progressive distillation (Salimans & Ho, ICLR 2022, Algorithm 2): training an N-step sampler from a 2N-step one (csrc/distill.hip) ----
 * The grid is the one of GeneralizedDDIM(..., "linear"): tau = linear_tau(T, 2N); student index i in 1..N stands for the timesteps
 * t = tau[2i], m = tau[2i-1], e = tau[2i-2].  One training step: z_t = alpha_t x0 + sigma_t eps; the frozen teacher at (z_t, t) gives the x0
 * estimate x1; one DDIM step z_m = alpha_m x1 + (sigma_m / sigma_t)(z_t - alpha_t x1); the teacher at (z_m, m) gives x2; the student
 * regresses at (z_t, t) on the x~ for which ONE DDIM step from z_t lands where the teacher's second step does.  The paper's quotient
 * (z_e - r z_t) / (alpha_e - r alpha_t), r = sigma_e / sigma_t, subtracts nearly equal numbers (1.3e-3 off in fp32 at T = 1000, N = 256) and
 * is never formed, and neither is z_e: substituting the two steps gives x~ = w1 x1 + w2 x2, w1 = (s_m - s_t) / (s_e - s_t),
 * w2 = (s_e - s_m) / (s_e - s_t), s = alpha / sigma, both positive with sum 1, (0, 1) where e = 0.
 * rows: device fp32 table [N+1][12], folded by the host in float64 from alpha_bar and rounded once; row 0 is NaN; row i:
 *   p0 p1    x1 = p0 o1 + p1 z_t    eps: (-sigma/alpha, 1/alpha), x0: (1, 0), v: (-sigma, alpha), all at t
 *   p0' p1'  x2 = p0' o2 + p1' z_m  the same at m
 *   m0 m1    z_m = m0 x1 + m1 z_t   m1 = sigma_m / sigma_t, m0 = alpha_m - m1 alpha_t
 *   w1 w2    x~ = w1 x1 + w2 x2
 *   q0 q1    target = q0 x~ + q1 z_t   eps: (-alpha/sigma, 1/sigma), x0: (1, 0), v: (-1/sigma, alpha/sigma), all at t
 *   two spare floats (0)
 * tt: device int64 table [N+1][2] = (t, m).  idx: int64[B] in DEVICE memory, one student index per image.  An index outside 1..N is never
 * used as an address: its image comes out NaN.  Every product and sum is rounded to fp32 on its own (no fma).  16-byte accesses where
 * chw % 4 == 0 and the image pointers are 16-byte aligned, element by element otherwise (any chw).
 * dmme_distill_noise: z_t = (sqrt_abar[t] x0) + (sqrt_1m_abar[t] z) at t = tt[idx_b][0] - dmme_q_sample's x_t, the same bits - and the
 *   two timestep vectors the teacher's forwards read, t_out[b] = t, m_out[b] = m (0 for a bad index); status[0] = 1 where an index lies
 *   outside 1..N (never cleared here).
 * dmme_distill_mid: x1 from the teacher's output out1 at (z_t, t), clamped to [-1, 1] iff clip; then z_m.
 * dmme_distill_target: x1 by the same device function, x2 from out2 at (z_m, m) (clamped iff clip), x~ and the target of the
 *   parameterisation: four reads, one write.  pred (DMME_PRED_*) names what the rows were folded for; the kernels read the rows only. */
DMME_API int dmme_distill_noise(const float* x0, const float* z, const int64_t* idx, const int64_t* tt, const float* sqrt_abar, const float* sqrt_1m_abar,
                                int N, int B, int64_t chw, float* z_t, int64_t* t_out, int64_t* m_out, int* status, void* stream);
DMME_API int dmme_distill_mid(int pred, int clip, const float* z_t, const float* out1, const float* rows, const int64_t* idx, int N, int B, int64_t chw,
                              float* z_m, void* stream);
DMME_API int dmme_distill_target(int pred, int clip, const float* z_t, const float* out1, const float* z_m, const float* out2, const float* rows,
                                 const int64_t* idx, int N, int B, int64_t chw, float* target, void* stream);

/* ---- consistency distillation (Song, Dhariwal, Chen & Sutskever 2023, Algorithm 2; the discrete grid and boundary scalings of Latent
 * Consistency Models, Luo et al. 2023): one training run, then 1-, 2- or 4-step samplers from the same weights (csrc/consistency.hip) ----
 * The grid is tau = linear_tau(T, N); index i in 1..N stands for t = tau[i], m = tau[i-1] (m = 0 exactly when i = 1).  With
 * sd = sigma_data, s = timestep_scaling:  cs(t) = sd^2 / ((s t)^2 + sd^2),  co(t) = s t / sqrt((s t)^2 + sd^2),  cs(0) = 1, co(0) = 0;
 *   x0(z, t; o) = p0 o + p1 z                     the x0 estimate of a network output o at the image z (clamped to [-1, 1] iff clip)
 *   f(z, t; o)  = cs(t) z + co(t) x0(z, t; o)      the consistency function: f(z, 0; .) = z
 * One step: z_t and the two timestep vectors (dmme_distill_noise), the frozen teacher at (z_t, t), one DDIM step to zh_m
 * (dmme_distill_mid), the target network at (zh_m, max(m, 1)), f_target = f(zh_m, m; .) (dmme_cm_target), the student at (z_t, t), and
 * loss = (1/B) sum_b d(f(z_t, t; student)_b, f_target_b) with its gradient with respect to the student's raw output (dmme_cm_loss).
 * rows: device fp32 table [N+1][12], folded by the host in float64 from alpha_bar and rounded once; row 0 is NaN; row i:
 *   p0 p1    x0 at t:  eps: (-sigma/alpha, 1/alpha), x0: (1, 0), v: (-sigma, alpha)
 *   p0' p1'  the same at the true m; (-0 or 0, 1) at m = 0, with no division by sigma anywhere
 *   m0 m1    zh_m = m0 x1 + m1 z_t   m1 = sigma_m / sigma_t, m0 = alpha_m - m1 alpha_t; (1, 0) at m = 0
 *   cs co    at t
 *   cs' co'  at the true m; (1, 0) at m = 0
 *   two spare floats (0)
 * The first six slots and tt, int64 [N+1][2] = (t, max(m, 1)), have the layout dmme_distill_noise and dmme_distill_mid read; column 1 is
 * the timestep the target network is evaluated at, the rows are what carry m = 0.  idx: int64[B] in DEVICE memory.  An index outside 1..N
 * is never used as an address: its image of f_target and d_out comes out NaN, and so does the loss.  Every fp32 product and sum is rounded
 * on its own (no fma); both sides of the loss go through one device function f.  16-byte accesses where chw % 4 == 0 and the image
 * pointers are 16-byte aligned, element by element otherwise (any chw).
 * dmme_cm_target: f_target = (cs' z_m) + (co' x0'), x0' = (p0' out_m) + (p1' z_m) clamped iff clip.
 * dmme_cm_loss: S_b = sum_j (f - f_target)_j^2 over image b, f = (cs z_t) + (co x0) from the student's raw output `out` (never clamped).
 *   metric DMME_CM_PSEUDO_HUBER: d_b = sqrt(S_b + c^2) - c,  g_b = grad_scale co p0 / (B sqrt(S_b + c^2))      (c > 0)
 *   metric DMME_CM_L2:           d_b = S_b / chw,           g_b = 2 grad_scale co p0 / (B chw)                  (c unused)
 *   loss[0] = (1/B) sum_b d_b;  sumsq (nullable, float[B]) = S_b;  d_out (nullable) = g_b (f - f_target).
 *   d_b and g_b are formed once per image from the device's own S_b, in double ((grad_scale co) p0 over B times the root), rounded once.
 *   Three plain launches, no atomics and no workgroup waiting for another: up to 64 workgroups per image leave partial sums in
 *   `scratch`, one workgroup adds them in index order and forms d_b, g_b and the loss, the gradient launch (only with d_out) reads g_b.
 *   `scratch` needs 65 * B floats.  B <= 65535.
 * dmme_ema_lerp: dst = (dst decay) + (src one_minus), one_minus = (float)(1.0 - (double)decay) formed on the host; decay in [0, 1]. */
enum { DMME_CM_PSEUDO_HUBER = 0, DMME_CM_L2 = 1 };
DMME_API int dmme_cm_target(int clip, const float* z_m, const float* out_m, const float* rows, const int64_t* idx, int N, int B, int64_t chw, float* f_target,
                            void* stream);
DMME_API int dmme_cm_loss(int metric, const float* z_t, const float* out, const float* f_target, const float* rows, const int64_t* idx, int N, int B,
                          int64_t chw, float c, float* loss, float* sumsq, float* d_out, float grad_scale, float* scratch, void* stream);
DMME_API int dmme_ema_lerp(float* dst, const float* src, int64_t numel, float decay, void* stream);

/* ---- Improved DDPM (learned variance): model_out is (B, 2C, H, W), channels [0, C) = eps, [C, 2C) = v
 * (IDDPM.forward_model, diffusion_models/iddpm.py:152-164); chw = C*H*W of ONE image of x. */

/* one reverse update, in place on x: replaces IDDPM.sampling_step after the model call
 * (diffusion_models/iddpm.py:118-150, equations/ddpm/ddpm.py:65-71, equations/iddpm/losses.py:34-37):
 *   mean = inv_sqrt_alpha * (x - eps_coef * eps);  std = sqrt(exp(v log_beta + (1 - v) log_beta_tilde));
 *   x = add_noise ? mean + std * z : mean.   log_beta_tilde = log(max(beta~_t, 1e-12)); add_noise = (t != 1). */
DMME_API int dmme_iddpm_step(float* x, const float* model_out, const float* z, float inv_sqrt_alpha, float eps_coef, float log_beta,
                    float log_beta_tilde, int add_noise, int B, int64_t chw, void* stream);

/* hybrid / VLB training loss and its gradient w.r.t. model_out: replaces the loss side of IDDPM.training_step
 * (diffusion_models/iddpm.py:92-116) = eq.ddpm.simple_loss + gamma * eq.iddpm.loss_vlb (equations/iddpm/losses.py:40-98,
 * discrete NLL rows for t == 1, KL rows otherwise, stop-gradient on eps inside L_vlb).
 *   loss[0] = w_simple * L_simple + w_vlb * L_vlb, loss[1] = L_simple, loss[2] = L_vlb   (3 floats);
 *   d_out (optional, B x 2C x H x W) = grad_scale * d loss[0] / d model_out.
 * t: int64[B] per-sample timesteps; coef: device fp32 table of 8 floats per timestep evaluated on the host with the
 * reference's fp32 torch ops: {1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), log beta_t, log max(beta~_t, 1e-12),
 * sqrt(abar_{t-1}) beta_t/(1-abar_t), sqrt(alpha_t)(1-abar_{t-1})/(1-abar_t), sqrt(beta~_t), 0}.
 * target: the noise re-derived by dmme_q_sample.  `scratch` needs 1024 floats. */
DMME_API int dmme_iddpm_loss(const float* model_out, const float* x_t, const float* x_0, const float* target, const int64_t* t,
                    const float* coef, int B, int64_t chw, float w_simple, float w_vlb, float* loss, float* d_out,
                    float grad_scale, float* scratch, void* stream);

/* ---- Improved DDPM as published (Nichol & Dhariwal 2021): per-image loss rows for importance-weighted L_vlb and for bits/dim, the prior
 * term of the bound, and the loss-second-moment timestep resampler (section 3.3).  These entry points take T and never use a device-side
 * value as an index before checking it against the table it indexes. */

/* dmme_iddpm_loss with per-image rows, optional importance weights and a checked t.  Per element the arithmetic is dmme_iddpm_loss's.
 *   rows[0][b] = S_b = mean over image b of (target - eps)^2
 *   rows[1][b] = V_b = mean over image b of the VLB term (discrete NLL where t[b] == 1, KL elsewhere), in nats/dim
 *   rows[2][b] = w_simple S_b + w_vlb V_b                                   (rows: 3 x B floats)
 *   loss[1] = mean_b S_b, loss[2] = mean_b V_b (both unweighted), loss[0] = (1/B) sum_b weight[b] rows[2][b]   (3 floats)
 *   d_out (optional, B x 2C x H x W) = what dmme_iddpm_loss writes, times weight[b].  weight == NULL stands for all ones and skips the
 *   multiply: d_out is then bit-identical to dmme_iddpm_loss's.
 * A t[b] outside [1, T] reads no row of coef: rows[.][b], loss[0..2] and image b of d_out become NaN and *status (nullable, device int) is
 * set to 1, as by dmme_log_softmax_grad.  Two launches, no atomics: up to 32 workgroups per image leave partial sums in `scratch`
 * (64 * B floats), one workgroup adds them in index order, so equal inputs give equal bits.  chw is free (no multiple of 4 needed). */
DMME_API int dmme_iddpm_loss_rows(const float* model_out, const float* x_t, const float* x_0, const float* target, const int64_t* t,
                                  const float* coef, int T, const float* weight, int B, int64_t chw, float w_simple, float w_vlb, float* loss,
                                  float* rows, float* d_out, float grad_scale, int* status, float* scratch, void* stream);

/* prior term of the variational bound, KL(q(x_T | x_0) || N(0, I)) per image in nats/dim:
 *   prior[b] = mean over image b of 0.5 (-log(1 - abar_T) - 1 + (1 - abar_T) + abar_T x_0^2),   0 <= alpha_bar_T < 1.
 * The three constant terms are folded on the host in double (they cancel to about abar_T^2 / 2). */
DMME_API int dmme_iddpm_prior_rows(const float* x_0, int B, int64_t chw, float alpha_bar_T, float* prior, void* stream);

/* draw t[B] and weight[B] from the loss history.  Caller-owned device state: hist float[T+1][H] (row 0 unused), count int32[T+1].
 *   warm  iff count[t] == H for every t in 1..T
 *   p[t]  = 1/T while not warm; else (1 - uniform_prob) s_t / sum(s) + uniform_prob / T with s_t = sqrt(mean_k hist[t][k]^2)
 *           (also 1/T where sum(s) is not a positive finite number).  p: float[T+1] output, p[0] = 0.
 *   u_b   = uniform b of the Philox span (philox_seed, philox_offset in quads): word b % 4 of quad b / 4, ((x >> 8) + 1) / 2^24
 *   t[b]  = 1 + #{t : cdf_t <= u_b cdf_T}, cdf the inclusive fp32 prefix sum of p, clamped to [1, T]: 1..T inclusive - T is reachable,
 *           unlike under the reference's uniform_int(1, T), or a history would never fill
 *   weight[b] = 1 / (T p[t[b]]); exactly 1.0f while not warm.
 * One workgroup (scan, then bisection); the prefix sums live in LDS: T <= 12288, DMME_ERR_UNSUPPORTED above. */
DMME_API int dmme_tsampler_draw(const float* hist, const int* count, int T, int H, float uniform_prob, uint64_t philox_seed,
                                uint64_t philox_offset, int B, int64_t* t, float* weight, float* p, void* stream);

/* push (t[b], L[b]), b = 0..B-1, into the history, with the result of doing so in index order: count[t] < H: hist[t][count[t]++] = L;
 * otherwise row t moves left by one and hist[t][H-1] = L.  Values are copied, never recomputed.  One thread owns each timestep and walks
 * the batch, so a timestep that occurs many times (more than H times too) needs no atomics.  An entry whose t[b] is outside [1, T] or
 * whose L[b] is not finite is skipped (a NaN in the history would poison p for good) and sets *status (nullable, device int) to 1. */
DMME_API int dmme_tsampler_update(float* hist, int* count, int T, int H, const int64_t* t, const float* L, int B, int* status, void* stream);

/* ---- Analytic-DPM (Bao et al., ICLR 2022): the statistic behind the optimal reverse variance of a fixed-variance noise prediction network,
 * and the rows of the K-step variational bound of such a network.  Both entry points follow dmme_iddpm_loss_rows and dmme_pf_dot: two plain
 * launches, no atomics; up to 32 workgroups per image leave partial sums in `scratch` (32 * B floats), one workgroup adds them in index
 * order in double, so equal inputs give equal bits.  chw is free (no multiple of 4 needed).  model_out holds image b's noise prediction in
 * the first chw values from b * image_stride: image_stride = chw for a DDPM network, 2 chw for an IDDPM network (the eps plane; v is not read).
 * A device-side index is checked before it indexes anything; a bad one sets *status (nullable, device int) to 1 and poisons its image only. */

/* m_b = (1/chw) sum_j eps[b][j]^2: fp32 products summed by fma, the partial sums and the division in double.  Then ONE thread walks
 * b = 0 .. B-1 in order: sum[t_b] += m_b, count[t_b] += 1 (sum: double[T+1], count: int64[T+1], entry 0 unused), so a timestep that occurs
 * twice in a batch has one well-defined result.  rows (nullable, float[B]) = (float) m_b.  A t_b outside [1, T] adds nothing, gives
 * rows[b] = NaN and sets *status. */
DMME_API int dmme_analytic_moment(const float* model_out, int64_t image_stride, const int64_t* t, int T, int B, int64_t chw, double* sum, int64_t* count,
                                  float* rows, int* status, float* scratch, void* stream);

/* rows[b] = term idx_b of the variational bound of the reverse process  p(x_{tau_{i-1}} | x_{tau_i}) = N(k0 x_t + k1 eps_theta, sigma_i^2 I)
 * against the posterior  q = N(k0 x_t + k1 eps, lambda_i^2 I), per image in nats/dim.  coef: device fp32 table of 8 floats per index
 * i = 0 .. S (row 0 unused): {k0_i, k1_i, log sigma_i^2, log lambda_i^2, sqrt(abar_tau_i), sqrt(1 - abar_tau_i), 0, 0}.
 * eps is re-derived from x_t and x_0 by dmme_q_sample's own expression, (x_t - sqrt(abar) x_0) / sqrt(1 - abar), from columns 4 and 5.
 *   idx_b >= 2: 0.5 (log sigma^2 - log lambda^2 + (lambda^2 + m_b) / sigma^2 - 1), m_b the mean over the image of (k1 (eps - eps_theta))^2:
 *               fp32 per element, summed by fma; the mean and the closing expression in double from the fp32 columns, rounded once.
 *   idx_b == 1: the mean of the discretised-Gaussian NLL of x_0, bins of width 2/255, open at +-1: per element the fp32 expressions of
 *               dmme_iddpm_loss at t == 1, in its order, with mean = (k0 x_t) + (k1 eps_theta) and sd = sqrt(exp(log sigma^2)).
 * An idx_b outside [1, S] reads no row, gives rows[b] = NaN and sets *status.  log lambda^2 = -inf (eta = 0) gives +inf above index 1. */
DMME_API int dmme_analytic_vlb_rows(const float* model_out, int64_t image_stride, const float* x_t, const float* x_0, const int64_t* idx, const float* coef, int S,
                                    int B, int64_t chw, float* rows, int* status, float* scratch, void* stream);

/* ---- single-op entry points used by the unit parity tests ---------------------------
 * Activations here are NHWC in the compute dtype; weights in the packed layout
 * [Cout][taps][Cin]; they exercise exactly the kernels the plan launches.
 * force_generic = 1 selects the shape-generic kernel instead of the MFMA kernel. */
typedef struct {
    int dtype;         /* dmme_dtype of activations / weights */
    int N, Hin, Win;   /* source dims (before the optional nearest 2x upsample) */
    int C1, C2;        /* channels of source 1 and (concat) source 2; C2 = 0: none */
    int upsample;      /* 1: nearest 2x upsample fused in front of the conv */
    int stride;        /* 1 or 2 */
    int taps;          /* 9: 3x3 pad 1; 1: 1x1 pad 0 */
    int Cout;
    int pro_silu;      /* SiLU after the affine prologue */
    int out_silu;      /* SiLU on the output */
    int nt;            /* rows of tproj (1 or N); 0: no time-embedding add */
    int tproj_ld;      /* leading dimension of tproj */
    int in_nchw;       /* src1 is fp32 NCHW (network input) */
    int out_nchw;      /* dst is fp32 NCHW (network output) */
    int force_generic;
} dmme_conv_desc;

DMME_API int dmme_conv2d(const dmme_conv_desc* d, const void* src1, const void* src2, const void* weight,
                const float* bias, const float* scale, const float* shift, const float* dmask,
                const float* tproj, const void* res1, const void* res2, int R1, void* dst, void* stream);

/* The second half of a channel-changing ResBlock as ONE launch (models/ddpm.py:108-111,131: `conv2(act(h)) + residual(x)`): the 3x3 conv
 * of dmme_conv2d over src1 (++ src2) with its prologue, plus the block's 1x1 residual conv over the RAW block input r_src1 [.., r_C1]
 * (++ r_src2 [.., r_C2]) with r_weight packed [Cout][r_C1 + r_C2] and r_bias [Cout], accumulated into the same output tile - no
 * residual tensor.  16-bit dtypes, stride 1, the shapes the wave-specialised kernel's 256-pixel form takes (whole 128-cout tiles,
 * r_C1 a multiple of 64, r_C1 + r_C2 a multiple of 128 and <= 512); DMME_ERR_UNSUPPORTED otherwise - it never falls back. */
DMME_API int dmme_conv2d_res(const dmme_conv_desc* d, const void* src1, const void* src2, const void* weight, const float* bias,
                const float* scale, const float* shift, const float* dmask, const void* r_src1, const void* r_src2, int r_C1,
                int r_C2, const void* r_weight, const float* r_bias, void* dst, void* stream);

/* GroupNorm statistics folded with the affine: scale[n][c] = rstd*gamma[c],
 * shift[n][c] = beta[c] - mean*rstd*gamma[c]  (nn.GroupNorm(eps=1e-5), models/ddpm.py:17-18). */
DMME_API int dmme_groupnorm_scale_shift(int dtype, const void* src1, const void* src2, int N, int HW, int C1, int C2,
                               int groups, const float* gamma, const float* beta, float eps, float* scale,
                               float* shift, float* partial_scratch, int force_generic, void* stream);

/* single-head self-attention over S tokens: qkv [N][S][3C] -> out [N][S][C]
 * softmax(q (k*C^-0.5)^T) v   (Attention.forward_attention, models/ddpm.py:54-63). */
DMME_API int dmme_attention(int dtype, const void* qkv, int N, int S, int C, void* out, int force_generic, void* stream);
/* The rest of the block in the same launch: dst = res + proj(attention(qkv)) (Attention.forward, models/ddpm.py:66-75, behind the
 * norm + qkv conv): w [C][C] (16-bit, the packed 1x1 layout: row = cout), bias [C] fp32, res / dst [N][S][C].  ctx (nullable):
 * also receives the attention output [N][S][C] (the proj conv's input, which its weight gradient needs).  gn_part (nullable):
 * (mean, M2) of dst per (image, 32-token tile, group of gn_cg = 4 or 8 channels), [N][S/32][C/gn_cg][2] fp32 - the partials the
 * next GroupNorm is finished from.  16-bit dtypes, S = 256, C = 128 or 256, N >= 128; DMME_ERR_UNSUPPORTED otherwise. */
DMME_API int dmme_attention_proj(int dtype, const void* qkv, int N, int S, int C, const void* w, const float* bias, const void* res,
                                 void* dst, void* ctx, float* gn_part, int gn_cg, void* stream);
/* The whole block `res + proj(attention(qkv(norm(x))))` in one launch, without a qkv tensor (weights fixed over a sampling chain).
 * dmme_attention_fold: wqkv [3C][C] / wp [C][C] 16-bit (packed 1x1 layout), bqkv [3C] / bp [C] fp32 -> M, wpv [C][C] 16-bit and
 *   c, bias2 [C] fp32 as dmme_unet_pack_folded defines them (bk drops out of a softmax over the keys).
 * dmme_attention_block: x, res, dst [N][S][C] 16-bit.  The norm comes as partials - parts [N][part_tiles][groups] {mean, M2} of
 *   part_cnt elements each, gamma / beta [C], eps; scale / shift [N][C] (nullable) then receive its rows - or, parts NULL, as the rows
 *   scale / shift themselves.  gn_part / gn_cg as dmme_attention_proj.  16-bit dtypes, S = 256, C = 128 or 256, any N >= 1. */
DMME_API int dmme_attention_fold(int dtype, int C, const void* wqkv, const float* bqkv, const void* wp, const float* bp, void* M, float* c, void* wpv,
                                 float* bias2, void* stream);
DMME_API int dmme_attention_block(int dtype, const void* x, int N, int S, int C, const float* parts, int part_tiles, int part_cnt, int groups,
                                  const float* gamma, const float* beta, float eps, float* scale, float* shift, const void* M, const float* c,
                                  const void* wpv, const float* bias2, const void* res, void* dst, float* gn_part, int gn_cg, void* stream);

/* multi-head self-attention exactly as the reference ships it (MultiHeadAttention.forward_attention,
 * models/iddpm.py:35-47): qkv [N][S][3C]; head h of image n reads channels [h*3d, (h+1)*3d) as (q | k | v), d = C/heads;
 * K is scaled by C^-0.5; result row n*heads + h is written to out[(n*heads + h) % N][S][((n*heads + h) / N)*d ...]
 * (the reference's "(b head)" split merged back as "(head b)").  heads = 1 equals dmme_attention. */
DMME_API int dmme_attention_heads(int dtype, const void* qkv, int N, int S, int C, int heads, void* out, int force_generic, void* stream);

/* NCHW fp32 <-> NHWC compute-dtype converters (test plumbing for the single-op calls) */
DMME_API int dmme_nchw_to_nhwc(int dtype, const float* src, int N, int C, int HW, void* dst, void* stream);
DMME_API int dmme_nhwc_to_nchw(int dtype, const void* src, int N, int C, int HW, float* dst, void* stream);
/* reference-layout fp32 weight (Cout, Cin, k, k) -> packed [Cout][k*k][Cin] in dtype */
DMME_API int dmme_pack_weight(int dtype, const float* src, int Cout, int Cin, int taps, void* dst, void* stream);

/* diagnostic: device buffer of >= 128 int64 that the wave-specialised conv kernel launched through dmme_conv2d fills
 * with shader-clock stamps of consumer wave 0 of workgroup 0: [0..63] arrive / leave of every stage barrier,
 * [64..87] the epilogue passes (tools/stamp_ws.py); NULL switches it off. */
DMME_API int dmme_debug_set_stamps(void* buf);

/* timing helper: records a HIP event pair around nothing; used by bench.py to time
 * on the launch stream.  Returns elapsed ms between two events created by the lib. */
DMME_API int dmme_event_create(void** ev);
DMME_API int dmme_event_record(void* ev, void* stream);
DMME_API int dmme_event_elapsed_ms(void* start, void* stop, float* ms);
DMME_API int dmme_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* DMME_HIP_H */
