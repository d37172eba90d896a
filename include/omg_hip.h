/*
 * omg_hip.h — C ABI of libomg_hip.so: the MI355X (gfx950) kernels behind OMG's
 * two-stage SDXL denoising hot path (boundary row B5).
 *
 * The reference (kongzhecn/OMG) is pure Python with no native code; its FFI for
 * this path is "torch ops called from diffusers modules".  Each entry point
 * below names the reference call site (file:line under /root/reference, or the
 * diffusers==0.25.0 symbol that call site dispatches to) that it replaces.
 *
 * Conventions (all entry points)
 *   - return 0 on success, a negative OMG_E* code on error; never throw,
 *     never allocate, never synchronise, never touch the host heap: safe under
 *     hipGraph capture.
 *   - every pointer is a DEVICE pointer owned by the caller; sizes are in
 *     elements of the named dtype unless suffixed _bytes.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 *   - `dtype` is OMG_F16 or OMG_BF16: the storage type of activations and
 *     weights.  All contractions accumulate in fp32 on MFMA.
 *   - activations inside the UNet are NHWC ("pixels × channels", i.e. the
 *     (B, H*W, C) token layout the transformer blocks want); the NCHW latent
 *     layout of the reference exists only at conv_in / conv_out.
 */
#ifndef OMG_HIP_H
#define OMG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMG_ABI_VERSION 6

enum { OMG_F16 = 0, OMG_BF16 = 1, OMG_F32 = 2 /* only where a signature says so */ };

enum {
  OMG_OK = 0,
  OMG_EINVAL = -1,   /* bad shape / alignment / null pointer          */
  OMG_EDTYPE = -2,   /* unsupported dtype                              */
  OMG_ELAUNCH = -3   /* hipLaunchKernel reported an error              */
};

/* activation applied in the GEMM / conv epilogue */
enum {
  OMG_ACT_NONE = 0,
  OMG_ACT_SILU = 1,  /* x*sigmoid(x)   — TimestepEmbedding.act (diffusers embeddings.py) */
  OMG_ACT_GEGLU = 2  /* out[:, j] = h[:, j] * gelu(h[:, N/2 + j]); W rows pre-packed by omg_pack_geglu_rows */
};

int omg_abi_version(void);
/* message of the last failed call made by the CALLING thread (thread-local storage; valid until that thread's next failing call) */
const char* omg_last_error(void);

/* ------------------------------------------------------------------------
 * omg_gemm — C[M,N] = epi( A[M,K] · W[N,K]^T  (+ A2[M,K2] · W2[N,K2]^T) )
 *
 * Replaces every nn.Linear on the path: attn.to_q/to_k/to_v/to_out[0]
 * (src/pipelines/lora_pipeline.py:98-124), Transformer2DModel.proj_in/out,
 * FeedForward GEGLU + out Linear, ResnetBlock2D.time_emb_proj, TimestepEmbedding
 * (diffusers 0.25.0).  The second K-segment is the PEFT LoRA branch
 * `base(x) + s·B(A(x))` (concept_models.set_adapters, lora_pipeline.py:588-591)
 * folded into the same MFMA accumulator: A2 = x·A_c^T (rank-r), W2 = s·B_c.
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t dtype;
  int32_t M, N, K;            /* K % 8 == 0, N % 8 == 0                              */
  const void* A;  int64_t lda;
  const void* W;  int64_t ldw;
  /* optional LoRA segment (K2 == 0 disables) */
  const void* A2; int64_t lda2;
  const void* W2; int64_t ldw2;
  int32_t K2;
  int32_t a2_col_block;       /* >0: A2 column offset = (n / a2_col_block) * K2 (fused q|k|v) */
  /* per-sample ("group") selection.  M = groups * rows_per_group.            */
  int32_t groups;             /* >=1                                                  */
  int32_t rows_per_group;
  const int32_t* group_adapter; /* [groups] adapter id or -1 (no LoRA); NULL = id 0  */
  int64_t w_adapter_stride;   /* W_eff  = W  + id * stride (LoRA-down GEMM); 0 = shared */
  int64_t w2_adapter_stride;  /* W2_eff = W2 + id * stride                             */
  /* epilogue */
  const void* bias;           /* [N] or NULL                                          */
  const void* group_bias; int64_t ldgb; /* [groups, N] per-sample bias (temb) or NULL  */
  const void* residual; int64_t ldr;    /* [M, N_out] or NULL                          */
  int32_t act;                /* OMG_ACT_*                                            */
  float out_scale;            /* applied before the residual add                      */
  void* C; int64_t ldc;       /* [M, N_out]; N_out = N/2 for GEGLU else N             */
} omg_gemm_args;

int omg_gemm(const omg_gemm_args* a, void* stream);

/* The buffer-descriptor offset limit of the GEMM family, in bytes (host-only query, no GPU needed).
 *
 * The large-tile kernels behind omg_gemm, omg_conv2d, omg_conv2d_slots, omg_gemm_mx8 and omg_conv2d_mx8 reach every operand through
 * a buffer descriptor and a 32-bit byte offset.  They are used while the byte extent of EVERY operand — rows x leading dimension
 * x element size for A, W, C, the residual and the per-sample bias table; B*Hin*Win*C for an NHWC input; 4x the phase launch's rows
 * for the Y of upsample == 2; the scale arrays of the MX-fp8 entries — is BELOW this limit.
 *   - Below the limit: any tile kernel may run; all of them give the same bits.
 *   - At or beyond it: the 16-bit entries (omg_gemm, omg_conv2d, omg_conv2d_slots, upsample == 2 included) run their 128x128 kernel,
 *     which forms 64-bit addresses — the same bits again, for operands of any size the int32 row count allows.  The MX-fp8 entries
 *     (omg_gemm_mx8, omg_conv2d_mx8) have no such kernel: they return OMG_EINVAL and write nothing. */
int64_t omg_debug_gemm_offset_limit(void);

/* ------------------------------------------------------------------------
 * omg_quant_mx8 / omg_gemm_mx8 — the same Linear layers with OCP MX fp8
 * operands (BASELINE.json north_star "MFMA bf16/fp8", configs[4]): elements
 * e4m3, one E8M0 scale (2^(s-127)) per 32 consecutive K elements, contraction
 * on v_mfma_scale_f32_32x32x64_f8f6f4 (the 5 PFLOP/s path of gfx950), fp32
 * accumulation, fp16 / bf16 output with the epilogues of omg_gemm.
 *
 * Scale layout (both operands): uint32 S[K/128][ld]; S[t][r] packs the four
 * scale bytes of row r for K blocks 4t .. 4t+3 (byte b = block 4t + b).
 *
 * omg_quant_mx8: X[M,K] (fp16 / bf16, row stride ldx elements) -> Q[M,K]
 * bytes (row stride ldq) + S.  Scale = smallest power of two with
 * amax / scale <= 448 (no element saturates), clamped at 2^-127 (byte 0, also
 * the byte of a block of zeros).  K % 128 == 0, s_ld >= M.
 * Weights are quantised once with the same call (rows = output features).
 * Non-finite input (this and every other producer of the format):
 *  - A non-finite input element is stored as an e4m3 NaN byte (0x7f or 0xff).
 *  - Every block of the tensor that holds no non-finite element has exactly
 *    the bytes and scale byte it would have without it.
 *  - Within the affected block, the finite elements and the scale byte are
 *    unspecified.  The row's dot product is NaN regardless.
 * ---------------------------------------------------------------------- */
int omg_quant_mx8(int32_t dtype, const void* x, int64_t ldx, int32_t M, int32_t K,
                  void* q, int64_t ldq, void* scales, int32_t s_ld, void* stream);

typedef struct {
  int32_t dtype;              /* type of C, bias, residual: OMG_F16 | OMG_BF16        */
  int32_t M, N, K;            /* K % 128 == 0, N % 8 == 0                             */
  const void* A; int64_t lda; /* e4m3 bytes [M, K], lda % 16 == 0                     */
  const void* a_scale; int32_t sa_ld;   /* uint32 [K/128][sa_ld], sa_ld >= M          */
  const void* W; int64_t ldw; /* e4m3 bytes [N, K] (per adapter), ldw % 16 == 0       */
  const void* w_scale; int32_t sw_ld;   /* uint32 [K/128][sw_ld]                      */
  int32_t groups, rows_per_group;       /* as omg_gemm                                */
  const int32_t* group_adapter;         /* [groups] weight slot per sample or NULL    */
  int64_t w_adapter_stride;   /* bytes (= elements) between weight slots; 0 = shared  */
  int64_t sw_adapter_stride;  /* scale columns between weight slots (normally N)      */
  const void* bias;           /* [N] or NULL                                          */
  const void* residual; int64_t ldr;
  int32_t act;                /* OMG_ACT_NONE | OMG_ACT_SILU | OMG_ACT_GEGLU          */
  float out_scale;
  void* C; int64_t ldc;
  /* c_scale != NULL (GEGLU only, N % 256 == 0): the result is written as the NEXT omg_gemm_mx8's A operand instead of 16 bits —
   * C = e4m3 bytes [M][N/2] (ldc in bytes, % 16), c_scale = uint32 [N/2/128][sc_ld] — bit-identical to omg_quant_mx8 of the
   * 16-bit result (FeedForward: GEGLU -> Linear, diffusers attention.py). */
  void* c_scale; int32_t sc_ld;
} omg_gemm_mx8_args;

int omg_gemm_mx8(const omg_gemm_mx8_args* a, void* stream);

/* 3x3 / stride 1 / pad 1 convolution of an MX-fp8 NHWC feature map (omg_groupnorm_mx8's output) with MX-fp8 weights
 * (omg_quant_mx8 of the packed [Cout][ky][kx][Cin] weight, K = 9 Cin) on the block-scaled MFMA: the resnet convolutions
 * (conv1 with the time-embedding projection as per-sample bias, conv2 with the skip tensor as residual) of BASELINE configs[4].
 * Output, bias, group_bias and residual are fp16 / bf16 (`dtype`). */
typedef struct {
  int32_t dtype;
  int32_t B, H, W, Cin, Cout;        /* Cin % 128 == 0, Cout % 8 == 0                         */
  const void* X; const void* x_scale;      /* e4m3 [B*H*W][Cin]; uint32 [Cin/128][B*H*W]      */
  const void* Wq; const void* w_scale;     /* e4m3 [Cout][9*Cin]; uint32 [9*Cin/128][sw_ld]   */
  int32_t sw_ld, act;
  const void* bias;                  /* [Cout] or NULL                                        */
  const void* group_bias; int64_t ldgb;    /* [B][ldgb] per-sample bias or NULL               */
  const void* residual;              /* [B*H*W][Cout] or NULL                                 */
  float out_scale;
  void* Y;                           /* [B*H*W][Cout]                                         */
} omg_conv2d_mx8_args;
int omg_conv2d_mx8(const omg_conv2d_mx8_args* a, void* stream);

/* ------------------------------------------------------------------------
 * omg_conv2d — NHWC implicit-GEMM convolution (3x3 pad 1, or 1x1), stride 1|2,
 * optional fused nearest-2x upsample of the input and fused channel-concat of
 * two inputs (the UNet skip connection), same epilogues as omg_gemm.
 *
 * Replaces ResnetBlock2D.conv1/conv2/conv_shortcut, Downsample2D.conv,
 * Upsample2D (F.interpolate nearest + conv) and torch.cat([h, res], dim=1) in
 * CrossAttnUpBlock2D/UpBlock2D — all inside the `self.unet(...)` call at
 * src/pipelines/lora_pipeline.py:546-566 (diffusers 0.25.0 unet_2d_blocks.py).
 * W is [Cout][ky][kx][C1+C2] (packed by the host from the diffusers OIHW key).
 *
 * upsample == 2, the phase form: the same result as upsample == 1 up to rounding, with 4/9 of the multiplies.  Four output pixels
 * share each source pixel, so output pixel (2y+py, 2x+px) is a 2x2 convolution of the SOURCE image: tap (a, c), a, c in {0, 1},
 * reads source pixel (y-1+py+a, x-1+px+c) (zeros outside the image) with the sum of the 1, 2, 2 or 4 original taps that land on
 * it (py = 0: row y-1 with w[0], row y with w[1]+w[2]; py = 1: row y with w[0]+w[1], row y+1 with w[2]; the same along x).
 * W is then the phase-packed weight [4 phases][Cout][4*C1], phase 2*py+px, taps (a, c) row-major, each summed weight rounded
 * to the storage type once; the call is four launches of M = B*Hin*Win rows and K = 4*C1, each scattering its rows to its
 * phase's output pixels.  Refused with OMG_EINVAL, never replaced by another form: stride != 1, ksize != 3, X2 / C2, residual.
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t dtype;
  int32_t B, Hin, Win;        /* input spatial size (before upsample)                 */
  int32_t C1, C2;             /* channels of X1 and (optional) X2; both % 64 == 0     */
  int32_t Hout, Wout, Cout;   /* Cout % 8 == 0                                        */
  int32_t ksize;              /* 1 or 3                                               */
  int32_t stride;             /* 1 or 2                                               */
  int32_t upsample;           /* 1: conv runs on nearest-2x-upsampled input; 2: the same as four 2x2 phase convolutions (above) */
  const void* X1; const void* X2;
  const void* W;              /* [Cout][ksize*ksize*(C1+C2)]; upsample == 2: [4][Cout][4*C1] */
  const void* bias;           /* [Cout] or NULL                                       */
  const void* group_bias; int64_t ldgb; /* [B, Cout] per-sample bias (time emb) or NULL */
  const void* residual;       /* NHWC [B,Hout,Wout,Cout] or NULL                      */
  float out_scale;
  void* Y;                    /* NHWC [B,Hout,Wout,Cout]                              */
  int32_t act;                /* OMG_ACT_NONE | OMG_ACT_SILU (ControlNetConditioningEmbedding)  */
} omg_conv2d_args;

int omg_conv2d(const omg_conv2d_args* a, void* stream);

/* ------------------------------------------------------------------------
 * omg_conv2d_slots — omg_conv2d with a weight slot per sample and the LoRA
 * second K-segment: LoRA on convolution layers (LoCon / PEFT Conv2d).
 *
 * The reference loads concept and style LoRAs with pipe.load_lora_weights
 * (inference_lora.py:162-170, inference_instantid.py:220-222; diffusers 0.25 +
 * peft 0.8.2), which wraps Conv2d layers as readily as Linear ones:
 *   y = conv(x; W) + s * B(A(x)),  A: k x k conv Cin -> r with the base layer's
 *   stride and padding, B: 1x1 conv r -> Cout  (peft tuners/lora/layer.py Conv2d),
 * toggled per concept pass by set_adapters (lora_pipeline.py:340-342, :588-591).
 * Semantics follow omg_gemm's: a sample is a group (rows_per_group = Hout*Wout),
 * M tiles never straddle a sample.
 *   merged mode : conv.W = [1+S][Cout][K] (base, then W + s*B_s A_s), w_slot_stride = Cout*K, K2 = 0.
 *   segment mode: first the LoRA-down conv (conv.W = [S][r_pad][K], w_slot_stride = r_pad*K, Cout = r_pad; a sample whose
 *                 slot is -1 is skipped and its output rows are left untouched), then the base conv with w_slot_stride = 0,
 *                 A2 = the down result, W2 = [S][Cout][K2] = s*B: samples with slot >= 0 add A2 . W2[slot]^T into the SAME
 *                 accumulator before the epilogue (acc + bias + group_bias) * out_scale + residual, with the activation.
 * Without group_adapter every sample uses slot 0.  Slot values are read on the device and not range-checked.
 * conv.upsample == 2 (the phase form of omg_conv2d): every slot holds the phase image [4][Cout][4*C1] (w_slot_stride >= 4*Cout*4*C1
 * or 0); the LoRA K-segment (K2 > 0) is refused.
 * ---------------------------------------------------------------------- */
typedef struct {
  omg_conv2d_args conv;            /* exactly omg_conv2d's meaning                                  */
  const int32_t* group_adapter;    /* [B] weight slot of each sample; NULL = slot 0                 */
  int64_t w_slot_stride;           /* elements between weight slots of conv.W; 0 = one shared W     */
  const void* A2; int64_t lda2;    /* [B*Hout*Wout, K2] LoRA-down result (16-bit), or NULL          */
  const void* W2; int64_t ldw2;    /* [Cout, K2] per slot: s*B                                      */
  int64_t w2_slot_stride;          /* elements between slots of W2; 0 = shared                      */
  int32_t K2;                      /* K2 % 8 == 0; 0 disables the segment                           */
} omg_conv2d_slots_args;

int omg_conv2d_slots(const omg_conv2d_slots_args* a, void* stream);

/* ------------------------------------------------------------------------
 * omg_attn_fwd — softmax(Q K^T * scale) V, head_dim 64, never materialising
 * the probabilities, with prompt-to-prompt "probability borrowing".
 *
 * Replaces, in one kernel: attn.get_attention_scores (baddbmm + softmax),
 * the controller's in-place edit of the conditional half of the probabilities,
 * and torch.bmm(probs, value) — src/pipelines/lora_pipeline.py:114-116 with
 * src/prompt_attention/p2p_attention.py:28-40,124-138.  With mapper = I and
 * alpha = 1 (always, in OMG flows) the controller's
 * `probs[edit] := probs[base]` is "sample b attends with the Q,K of sample
 * qk_src[b] but its own V".  Also replaces F.scaled_dot_product_attention /
 * xformers in the concept UNet (src/ip_adapter/attention_processor.py:273,383,399)
 * — `accumulate` implements IPAttnProcessor2_0's `text + scale*ip` (:409).
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t dtype;
  int32_t B, heads, Nq, Nkv;  /* head_dim is 64                                       */
  const void* Q; int64_t ldq; int64_t q_bstride;   /* row stride / batch stride (elements) */
  const void* K; int64_t ldk; int64_t k_bstride;
  const void* Vt;             /* [B, heads, 64, Nkv_pad] from omg_transpose_v (its key order); columns >= Nkv MUST be zero (it writes
                                 them so): the kernels that read it mask no score, the padded keys cancel against those zeros.  May be
                                 NULL when V (below) is given and Nkv > 128 */
  int32_t Nkv_pad;            /* % 64 == 0                                            */
  const int32_t* qk_src;      /* device [B]: batch index supplying Q,K; NULL = identity */
  float scale;
  int32_t accumulate;         /* 0: O = out_scale*attn ; 1: O += out_scale*attn       */
  float out_scale;
  void* O; int64_t ldo; int64_t o_bstride;
  /* ABI 6: V ROW-MAJOR — [B, Nkv, (head, 64)] with row stride ldv and batch stride v_bstride (elements, both % 8 == 0), i.e. the V
   * columns of the fused QKV projection's output exactly as omg_gemm wrote them.  When given and Nkv > 128 (self-attention) the kernel
   * stages it like K and transposes on the LDS read (ds_read_b64_tr_b16): no omg_transpose_v pass, Vt / Nkv_pad may be NULL / 0.
   * With Nkv <= 128 pass Vt (the resident-K/V kernels want the V^T image); V alone is rejected there.  NULL = ABI 5 behaviour.
   * The row-major path addresses one (sample, head) slice of K / of V with 32-bit offsets: Nkv * ldk * 2 and Nkv * ldv * 2 bytes must stay below 2 GB
   * (OMG_EINVAL otherwise; 16 384 keys of a 3 840-wide fused projection are 126 MB). */
  const void* V; int64_t ldv; int64_t v_bstride;
} omg_attn_args;

int omg_attn_fwd(const omg_attn_args* a, void* stream);

/* omg_attn_fwd with a causal mask: key j is visible to query i iff j <= i and j < Nkv (top-left alignment; rows >= Nkv - 1 see
 * every key, every row sees key 0).  Replaces the causal self-attention of transformers' CLIPTextModel (CLIPAttention with
 * causal_attention_mask: bmm + additive -inf mask + softmax + bmm), which the reference reaches through encode_prompt for the global
 * prompt, its negative and one prompt pair per concept (src/pipelines/lora_pipeline.py:315-347).  Same argument struct and the same
 * meaning of qk_src, accumulate, out_scale and a strided O.  Served by the causal instance of the resident-K/V kernel only:
 *   Nkv <= 128 (OMG_EINVAL above: the self-attention kernel has no causal form);
 *   Vt from omg_transpose_v (mfma_key_order = 1, zero-padded columns) is required — row-major V alone is OMG_EINVAL;
 *   O 16-byte aligned, ldo and o_bstride multiples of 8 elements.
 * Scores and probabilities stay in fp32 and the mask is applied before the row maximum is taken, so a masked score of any size —
 * or a non-finite one, as long as K and V hold no NaN / inf — leaves the visible keys' result untouched bit for bit. */
int omg_attn_fwd_causal(const omg_attn_args* a, void* stream);

/* V[B, Nkv, (head, 64)] (row stride ldv) -> Vt[B, heads, 64, Nkv_pad], zero padded.  mfma_key_order = 1 (what omg_attn_fwd
 * consumes): inside every group of 16 keys the order is [0-3, 8-11, 4-7, 12-15] — the operand order of the P·V MFMA, one
 * 16-byte LDS read per lane; 0: natural key order (a plain batched transpose, used by the VAE / text-encoder attention). */
int omg_transpose_v(int dtype, const void* V, int64_t ldv, int64_t v_bstride,
                    int B, int heads, int Nkv, int Nkv_pad, void* Vt, int mfma_key_order, void* stream);

/* omg_transpose_v_mapped — the general prompt-to-prompt cross-attention edit, folded into V.
 *
 * Replaces AttentionReplace.replace_cross_attention and the alpha blend of AttentionControlEdit.forward
 * (src/prompt_attention/p2p_attention.py:131-133, :146-147: einsum('hpw,bwn->bhpn', base, mapper) * alpha + (1 - alpha) * own) for a
 * non-identity mapper (word swap) and for cross-replace windows, without the probability tensor: with P_b / P_e the base / edited
 * sample's probabilities,
 *     (P_b M_e * alpha_e + (1 - alpha_e) * P_e) V_e  =  P_b V'_e + P_e V''_e,
 *     V'_e[w, :] = sum_n M_e[w, n] alpha_e[n] V_e[n, :],    V''_e[n, :] = (1 - alpha_e[n]) V_e[n, :].
 * The caller runs omg_attn_fwd twice: qk_src = base on Vt_mapped, then the sample's own Q, K with accumulate = 1 on Vt_own.
 *
 * One launch for the whole batch.  Both outputs are [B, heads, 64, Nkv_pad] in omg_transpose_v's mfma_key_order = 1 layout, columns
 * >= Nkv written as zeros.  Row b with edit_of[b] < 0: Vt_mapped is the plain transpose (bit-equal to omg_transpose_v), Vt_own is
 * zero.  Other rows use tables edit_of[b] (clamped to E - 1) at step *step_idx (clamped to [0, steps - 1]; NULL = row 0): the step is
 * read on the device, so one captured graph serves every step.  fp32 accumulation over n, one rounding to dtype; a term whose
 * coefficient is exactly 0 is skipped, so inf / NaN in a V row that no coefficient selects does not reach the output.
 * OMG_EINVAL (nothing written): Nkv > 128, Nkv_pad % 64 != 0 or < Nkv, E <= 0, steps <= 0, ld_mapper < Nkv, V not 16-byte aligned
 * or ldv / v_bstride not multiples of 8 elements, outputs not 16-byte aligned, a NULL operand. */
typedef struct {
  int32_t dtype;                  /* OMG_F16 / OMG_BF16                                                        */
  int32_t B, heads, Nkv, Nkv_pad; /* head_dim is 64; Nkv <= 128; Nkv_pad % 64 == 0                             */
  const void* V; int64_t ldv; int64_t v_bstride;   /* [B, Nkv, (head, 64)] as omg_gemm wrote the [k|v] projection (elements) */
  const int32_t* edit_of;         /* device [B]: index into the tables, or -1 for a row that is not edited     */
  int32_t E, steps;
  const float* mapper; int64_t ld_mapper; int64_t mapper_estride;        /* M_e[w][n] = mapper[e * estride + w * ld + n]  */
  const float* alpha; int64_t alpha_step_stride; int64_t alpha_estride;  /* alpha[step * step_stride + e * estride + n]   */
  const int32_t* step_idx;        /* device scalar, or NULL                                                     */
  void* Vt_mapped; void* Vt_own;
} omg_vmap_args;

int omg_transpose_v_mapped(const omg_vmap_args* a, void* stream);

/* ------------------------------------------------------------------------
 * Normalisation.  GroupNorm (NHWC, fp32 statistics as sums shifted by a
 * per-channel pivot and merged as (mean, M2), so that |mean| >> std does not
 * cancel; deterministic two-stage reduction) replaces ResnetBlock2D.norm1/norm2 + nonlinearity, Transformer2D
 * .norm and UNet conv_norm_out + conv_act; LayerNorm replaces
 * BasicTransformerBlock.norm1/2/3 (diffusers 0.25.0 attention.py).
 * ---------------------------------------------------------------------- */
/* workspace: floats, at least omg_groupnorm_ws_floats(B, groups, HW) */
int64_t omg_groupnorm_ws_floats(int B, int groups, int HW);
/* X may be the channel-concat of X1 (C1) and X2 (C2) — pass X2=NULL,C2=0 otherwise */
int omg_groupnorm(int dtype, const void* X1, int C1, const void* X2, int C2,
                  int B, int HW, int groups, float eps,
                  const void* gamma, const void* beta, int silu,
                  float* workspace, void* Y, void* stream);
int omg_layernorm(int dtype, const void* X, int64_t ldx, int M, int C, float eps,
                  const void* gamma, const void* beta, void* Y, int64_t ldy, void* stream);
/* LayerNorm whose consumer is omg_gemm_mx8: the normalised row (rounded to `dtype` exactly as omg_layernorm stores it) is
 * written as MX-fp8 bytes Q[M, C] + stage-major scale dwords (layout of omg_quant_mx8).  C % 128 == 0. */
int omg_layernorm_mx8(int dtype, const void* X, int64_t ldx, int M, int C, float eps,
                      const void* gamma, const void* beta, void* Q, int64_t ldq,
                      void* scales, int s_ld, void* stream);

/* GroupNorm(+SiLU)(+concat) whose consumer is omg_conv2d_mx8 (the resnets' norm1 -> conv1, norm2 -> conv2, diffusers 0.25.0
 * resnet.py ResnetBlock2D.forward): y, rounded to `dtype` exactly as omg_groupnorm stores it, is written as MX-fp8 bytes
 * Q[B*HW][Cq] and per-pixel scales S[Cq/128][B*HW] dwords (byte j of a dword: the E8M0 scale of channels 128 k + 32 j .. + 31);
 * C = C1 + C2 must be a multiple of 32, Cq = C rounded up to a multiple of 128, and the Cq - C pad channels are written as
 * zeros with scale byte 0 (SDXL's 320- and 960-channel maps: Cq = 384, 1024; the convolution weight is padded alike). */
int omg_groupnorm_mx8(int dtype, const void* X1, int C1, const void* X2, int C2,
                      int B, int HW, int groups, float eps,
                      const void* gamma, const void* beta, int silu,
                      float* workspace, void* Q, void* scales, void* stream);

/* ------------------------------------------------------------------------
 * fp32 path of the VAE decode.  The reference upcasts the VAE before decoding ("it overflows in float16", upcast_vae at
 * src/pipelines/lora_pipeline.py:639-652); with torch 2's attention processor diffusers 0.25 then runs post_quant_conv, conv_in
 * and the mid block in fp16 and the UP BLOCKS, conv_norm_out and conv_out in fp32.  omg_conv2d_f32: NHWC fp32 convolution
 * (3x3 pad 1 or 1x1, stride 1, optional fused nearest-2x upsample of the input), fp32 weights [Cout][ky][kx][Cin], fp32 bias and
 * residual, on the f32-input MFMA (exact fp32 products, fp32 accumulation).  omg_groupnorm / omg_conv_out accept
 * dtype = OMG_F32 (fp32 storage, fp32 gamma / beta / weights); omg_cast_f32 is the decoder's `sample.to(upscale_dtype)`.
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t B, Hin, Win, Cin;   /* Cin % 32 == 0                                        */
  int32_t Hout, Wout, Cout;   /* Hout = Hin * (upsample ? 2 : 1); Cout % 4 == 0       */
  int32_t ksize, upsample;    /* X may exceed 4 GB: the kernel addresses it from the first image a 128-pixel tile touches; ONE image (Hin * Win * Cin * 4 bytes)
                                 must stay below ~2 GB and the packed weight below 2 GB (OMG_EINVAL otherwise) */
  const void* X; const void* W; const void* bias; const void* residual;   /* fp32; bias / residual may be NULL */
  void* Y;                    /* [B, Hout, Wout, Cout] fp32                           */
} omg_conv2d_f32_args;

int omg_conv2d_f32(const omg_conv2d_f32_args* a, void* stream);

/* The same 3x3 / stride 1 / pad 1 convolution as Winograd F(2x2, 3x3): 16 instead of 36 multiplies per 2x2 output tile and input
 * channel on the same MFMA (result equal to omg_conv2d_f32 to fp32 rounding, not bitwise).  U: the transformed weight G g G^T in
 * the kernel's streaming order, fp32 [ceil(Cout / 64)][Cin / 8][pos 16][k chunk 2][row 64][4]  (element: position pos = 4 i + j of
 * the 4x4 transform, output channel 64 block + row (zero beyond Cout), input channel 8 stage + 4 chunk + e);
 * omg_conv2d_f32_wino_weight_floats gives its size.  Hout and Wout must be even. */
typedef struct {
  int32_t B, Hin, Win, Cin;   /* Cin % 8 == 0                                         */
  int32_t Hout, Wout, Cout;   /* Hout = Hin (2 Hin with upsample), even; Cout % 4 == 0 */
  int32_t upsample;           /* 1: nearest-2x upsample of X fused into the gather    */
  const void* X; const void* U; const void* bias; const void* residual;   /* fp32; bias / residual may be NULL */
  void* Y;                    /* [B, Hout, Wout, Cout] fp32                           */
} omg_conv2d_f32_wino_args;

int64_t omg_conv2d_f32_wino_weight_floats(int Cout, int Cin);
int omg_conv2d_f32_wino(const omg_conv2d_f32_wino_args* a, void* stream);
int omg_cast_f32(int dtype, const void* X, float* Y, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * Boundary convolutions (NCHW latents <-> NHWC features).
 * conv_in : UNet2DConditionModel.conv_in  (4 -> C0, 3x3), input NCHW fp32|T; executed as a 64-column
 *           im2col + the MFMA GEMM (K = 36 padded to one 64-wide slice).
 * conv_out: UNet2DConditionModel.conv_out (C0 -> 4, 3x3) on the already
 *           normalised+SiLU'd NHWC features, output NCHW in fp32.
 * ---------------------------------------------------------------------- */
int omg_conv_in(int dtype, const void* X_nchw, int x_is_f32, int B, int Cin, int H, int W,
                const void* Wt /*[Cout][64]: (ky,kx,ci) order, zero padded to 64 columns*/, const void* bias, int Cout,
                void* workspace /* B*H*W*64 elements of dtype: im2col patches */,
                void* Y_nhwc, void* stream);
int omg_conv_out(int dtype, const void* X_nhwc, int B, int H, int W, int Cin,
                 const void* Wt /*[Cout][3][3][Cin]*/, const void* bias, int Cout,
                 float* Y_nchw, void* stream);

/* ------------------------------------------------------------------------
 * Small elementwise pieces of the time/text conditioning path
 * (diffusers embeddings.py get_timestep_embedding, flip_sin_to_cos=True,
 *  downscale_freq_shift=0; and `self.nonlinearity(temb)` in ResnetBlock2D).
 * ---------------------------------------------------------------------- */
int omg_timestep_embedding(int dtype, const float* t, int n, int dim, void* out, int64_t ldo, void* stream);
int omg_silu(int dtype, const void* x, void* y, int64_t n, void* stream);
/* y[i] += a[i]  (ControlNet residuals added to the UNet skip tensors: `sample += residual`,
 * diffusers unet_2d_condition.py, reached from lora_pipeline.py:546-556) */
int omg_add_inplace(int dtype, void* y, const void* a, int64_t n, void* stream);
/* ------------------------------------------------------------------------
 * VAE decode (row N1): the two pieces AutoencoderKL.decode needs beyond the UNet's kernels
 * (diffusers 0.25.0 models/autoencoder_kl.py `post_quant_conv`, models/attention_processor.py
 * `Attention` with ONE head of dim C over all H*W tokens; reached from lora_pipeline.py:635-661).
 *   omg_softmax_rows : X[r, 0:cols] = softmax(X[r, 0:cols] * scale) in place, fp32 math, rows of `ld` elements
 *                      (the (HW x HW) score matrix of the mid-block attention, produced and consumed by omg_gemm).
 *   omg_channel_mix  : NCHW fp32, Y[b, o, p] = bias[o] + sum_c Wm[o, c] * X[b, c, p]   (1x1 conv, Cin, Cout <= 8)
 * ---------------------------------------------------------------------- */
int omg_softmax_rows(int dtype, void* X, int64_t rows, int64_t cols, int64_t ld, float scale, void* stream);
int omg_channel_mix(const float* X, const float* Wm, const float* bias, int B, int Cin, int Cout, int64_t HW,
                    float* Y, void* stream);
/* dst[r, col0 : col0+cols] = src[r, 0:cols]  (row-wise copy with strides, elements) */
int omg_copy2d(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, void* stream);

/* ------------------------------------------------------------------------
 * omg_fuse_cfg_step — region-masked noise fusion + classifier-free guidance +
 * scheduler update + next model input, one launch, zero host syncs.
 *
 * Replaces src/pipelines/lora_pipeline.py:568-607 (fusion, incl. get_region_mask
 * :674-681 and the nearest mask resize), :610-612 (CFG), :615 (scheduler.step)
 * and :491-492 (cat + scale_model_input of the next iteration); identical block
 * in src/pipelines/instantid_pipeline.py:618-707.
 *
 * noise_pred : fp32 [4,C,H,W] = [unc0, unc1, cond0, cond1]
 * region_pred: K pointers to fp32 [2,C,H,W] = [unc, cond] (NULL entry = concept without a mask)
 * masks      : K pointers to fp32 [Hm,Wm] full-resolution {0,1} masks (NULL = None)
 * coef       : device table [n_steps][4] = {cx, ce, cin_next, unused}; row = *step_idx
 *              latents' = cx*latents + ce*eps ; model_input' = cin_next * latents'
 * step_idx   : device int; read, and incremented when `advance` != 0
 * ---------------------------------------------------------------------- */
#define OMG_MAX_CONCEPTS 8
typedef struct {
  int32_t C, H, W;            /* latent channels (4) and size                         */
  int32_t Hm, Wm;             /* mask size (e.g. 1024 x 1024)                          */
  int32_t n_concepts;
  int32_t fuse;               /* 0: plain CFG step; 1: masked fusion (i > 15, stage 2) */
  float guidance_scale;
  const float* noise_pred;
  const float* region_pred[OMG_MAX_CONCEPTS];
  const float* masks[OMG_MAX_CONCEPTS];
  const float* coef;
  int32_t* step_idx;
  int32_t advance;
  float* latents;             /* fp32 [2,C,H,W], updated in place                     */
  int32_t out_dtype;          /* dtype of model_input_next                            */
  void* model_input_next;     /* [4,C,H,W] = cat([latents']*2) * cin_next  (may be NULL) */
  float* fused_noise_out;     /* optional fp32 [2,C,H,W]: the fused (unc1, cond1) — parity tap */
} omg_step_args;

int omg_fuse_cfg_step(const omg_step_args* a, void* stream);

/* omg_fuse_cfg_step_ms — the same fusion + CFG + next model input with a MULTISTEP scheduler update (DPM-Solver++,
 * omg_amd/schedulers.py DPMSolverMultistepScheduler).  a->coef is not read; instead
 * ms_coef : device table [n_steps][8] = {a, b, cx, cm, cp, cin_next, unused, unused}; row = *a->step_idx
 *             m = a*latents + b*eps                       (data prediction)
 *             latents' = cx*latents + cm*m + cp*m_prev ; model_input' = cin_next * latents'
 * x0_hist : fp32 [2,C,H,W] per request: m_prev of both samples on entry, this step's m on return.  Rows with cp == 0
 *           (order 1: the first step) do not read it, so it needs no initialisation. */
int omg_fuse_cfg_step_ms(const omg_step_args* a, const float* ms_coef, float* x0_hist, void* stream);

/* omg_fuse_cfg_step_noise — omg_fuse_cfg_step for a STOCHASTIC scheduler (Euler-ancestral, DDIM with eta > 0,
 * omg_amd/schedulers.py).  Reads the same table a->coef [n_steps][4], now with column 3 in use:
 *             row = {cx, ce, cin_next, cz}; latents' = cx*latents + ce*eps + cz*z ; model_input' = cin_next * latents'
 * z : fp32 Gaussian noise of this request, [2,C,H,W] per step; step s (= *a->step_idx, read on the device) is at
 *     z + s * z_step_stride (elements, >= 2*C*H*W).  Rows with cz == 0 do not read it. */
int omg_fuse_cfg_step_noise(const omg_step_args* a, const float* z, int64_t z_step_stride, void* stream);

/* out[0:n] = table[*step_idx * n : (*step_idx + 1) * n]: per-step conditioning (time/text embedding rows, hoisted out
 * of the loop by the host) selected with the DEVICE step counter, so a captured step graph has no host argument. */
int omg_gather_step(int dtype, const void* table, const int32_t* step_idx, void* out, int64_t n_per_step, void* stream);

/* model_input[4,C,H,W] (dtype) = cin * cat([latents]*2)  — first iteration of the loop */
int omg_scale_model_input(int dtype, const float* latents, const float* coef_cin, int n_per_sample, void* out, void* stream);

/* ------------------------------------------------------------------------
 * Protocol-mode pieces (materialised probabilities) so that ANY controller
 * object — including the reference's own AttentionReplace with a non-identity
 * mapper — can be driven through RegionControlNet_AttnProcessor's exact
 * sequence (lora_pipeline.py:114-116): scores -> softmax -> controller -> bmm.
 * ---------------------------------------------------------------------- */
/* P[bh, q, kv] = softmax_kv(scale * Q[bh,q,:] . K[bh,kv,:])   (Q/K as in omg_attn_fwd) */
int omg_attn_probs(const omg_attn_args* a, void* P /*[B*heads, Nq, Nkv] dtype*/, void* stream);
/* O[b, q, h*64+d] = sum_kv P[bh,q,kv] * V[b,kv,h*64+d] */
int omg_attn_apply_probs(int dtype, const void* P, const void* V, int64_t ldv, int64_t v_bstride,
                         int B, int heads, int Nq, int Nkv, void* O, int64_t ldo, int64_t o_bstride, void* stream);

/* ------------------------------------------------------------------------
 * EfficientViT LiteMLA (the segmentation hand-off between the two stages: /root/reference
 * src/efficientvit/models/nn/ops.py:335-455).  The qkv / grouped / proj 1x1 convolutions are omg_gemm launches; these are the rest.
 * omg_dwconv2d: depthwise ksize x ksize convolution of the multi-scale aggregation (ops.py:372-380), NHWC rows of ldx / ldy
 *   elements (so that it can read a column slice of the fused qkv buffer), weights [ksize*ksize][C] tap-major, stride 1, same padding.
 * omg_relu_linear_att: relu_linear_att (ops.py:405-441) in fp32 as the reference computes it.  QKV [B*HW][ld]: group g holds its
 *   q | k | v (dim each) at columns 3 dim g; OUT [B*HW][ldo]: group g at columns dim g.  dim in {8, 16, 32}.
 * omg_litemla_aggreg: one scale of the aggregation in one launch (ops.py:376-391): the depthwise convolution of omg_dwconv2d (fp32,
 *   rounded once to the storage dtype) and the 1x1 convolution with C / dim groups behind it on the 16-bit MFMA (fp32 accumulation,
 *   one rounding).  Wg [C][dim] is the grouped convolution's own weight.  dim in {16, 32}, C a multiple of dim.  Y may be another
 *   column slice of the buffer X is a slice of (ldx == ldy, disjoint columns); any other overlap is refused.
 * omg_dwconv2d and omg_relu_linear_att refuse a negative B, H, W or HW and return OMG_OK without a launch when B, H, W or HW is 0.
 *   Both do 16-byte accesses: X, the taps, bias (when given), Y, QKV and OUT must be 16-byte aligned (with ldx, ldy, ld, ldo
 *   multiples of 8 elements every row then is); the workspace holds floats.  omg_relu_linear_att writes every float of
 *   workspace[0 .. omg_relu_linear_att_ws_floats) before it reads it and touches none behind.
 * ---------------------------------------------------------------------- */
int omg_dwconv2d(int dtype, const void* X, int64_t ldx, int B, int H, int W, int C, int ksize,
                 const void* Wt, const void* bias, void* Y, int64_t ldy, void* stream);
int omg_litemla_aggreg(int dtype, const void* X, int64_t ldx, int B, int H, int W, int C, int ksize, int dim,
                       const void* Wt, const void* Wg, void* Y, int64_t ldy, void* stream);
int64_t omg_relu_linear_att_ws_floats(int B, int groups, int dim, int HW);
int omg_relu_linear_att(int dtype, const void* QKV, int64_t ld, int B, int HW, int groups, int dim, float eps,
                        float* workspace, void* OUT, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------
 * The convolutional part of the EfficientViT-SAM image encoder (omg_amd/efficientvit.py; the reference's
 * models/efficientvit/backbone.py and sam.py).  NHWC fp16 / bf16, BatchNorm folded into W and bias by the caller, fp32 accumulation,
 * one rounding.  Output size of both convolutions: (Hin - 1) / stride + 1 (kernel 3, padding 1).  GELU is the tanh form
 * (the reference's build_act("gelu") is nn.GELU(approximate="tanh")).
 * omg_conv3x3_nhwc_act: Y[B,Hout,Wout,Cout] = residual + gelu?(conv3x3(X[B,Hin,Win,Cin], W[Cout][3][3][Cin]) + bias), stride 1 | 2,
 *   an implicit GEMM on the 16-bit MFMA.  Cin % 8 == 0 or Cin < 8 (the RGB stem; K is zero-padded inside the kernel); Cout % 8 == 0.
 *   act: 0 | 1 (GELU); bias [Cout] and residual [B,Hout,Wout,Cout] may be NULL.
 * omg_dwconv3x3_act: depthwise 3x3, stride 1 | 2, rows of ldx / ldy elements, weights [9][C] tap-major, C % 8 == 0.
 *   act bit 0: GELU of the output; bit 1: GELU of the INPUT as it is read (the activation of the 1x1 convolution in front).
 * omg_upsample_add_nhwc: Y[B,Hout,Wout,C] (+)= bicubic resize of X[B,Hin,Win,C] as torch.nn.functional.interpolate(mode="bicubic",
 *   align_corners=False) computes it; accumulate == 0 overwrites Y, != 0 adds to it (sum in fp32, one rounding).  C % 8 == 0.
 * ---------------------------------------------------------------------- */
int omg_conv3x3_nhwc_act(int dtype, const void* X, int B, int Hin, int Win, int Cin, int Cout, int stride,
                         const void* Wt, const void* bias, int act, const void* residual, void* Y, void* stream);
int omg_dwconv3x3_act(int dtype, const void* X, int64_t ldx, int B, int Hin, int Win, int C, int stride,
                      const void* Wt, const void* bias, int act, void* Y, int64_t ldy, void* stream);
int omg_upsample_add_nhwc(int dtype, const void* X, int B, int Hin, int Win, int C, int Hout, int Wout,
                          int accumulate, void* Y, void* stream);

/* ------------------------------------------------------------------------
 * SAM's mask decoder (omg_amd/sam.py: the two-way transformer, output_upscaling, the hypernetwork product) and the reference's
 * EfficientViTSam.postprocess_masks (models/efficientvit/sam.py:225-241).  Linear layers are omg_gemm, LayerNorms omg_layernorm.
 * omg_attn_small: O[b, q, h d + :] = softmax_k(scale Q[b, q, h d + :] . K[b, k, h d + :]) V[b, k, h d + :] for head_dim d = 16 | 32
 *   (omg_attn_fwd is fixed at 64).  Rows of ldq / ldk / ldv / ldo elements and batches of *_bstride elements (multiples of 8, base
 *   pointers 16-byte aligned): a column slice of a projection buffer is a valid operand.  Any Nq, Nk >= 1.  Scores, the
 *   running-maximum softmax and P V are fp32; one rounding at the store.  No key row >= Nk is read or weighted.
 * omg_convt2x2_ln_gelu: the scatter half of ConvTranspose2d(kernel 2, stride 2).  G [B H W][ldg] is the omg_gemm of the NHWC input
 *   rows against the weight laid out [(dy, dx, cout)][cin] (4 Cout rows); Y [B, 2H, 2W, Cout] NHWC:
 *     Y[b, 2y + dy, 2x + dx, :] = act(LN?(G[(b, y, x), (2 dy + dx) Cout + :] + bias))
 *   LayerNorm over the Cout channels of a pixel (biased variance, fp32 statistics) when ln_gamma / ln_beta are given; act 0 | 1 =
 *   erf GELU (nn.GELU()).  Cout % 8 == 0.
 * omg_sam_mask_logits: logits[b, m, p] (fp32) = sum_c hyper[b, m, c] up[b, p, c]; hyper [B, M, C], up [B, P, C], M <= 4, C % 8 == 0,
 *   C <= 64.  One pass over `up`.
 * omg_sam_postprocess: low [N, Hl, Wl] fp32 -> bilinear (align_corners = False) to image_size x image_size -> crop [:in_h, :in_w]
 *   -> bilinear to out_h x out_w, as two torch.nn.functional.interpolate calls in fp32 compute it (the intermediate is recomputed
 *   per output pixel, not stored).  out_u8 == 0: out is fp32 [N, out_h, out_w]; 1: uint8, 1 where the value > threshold.
 * omg_relu: Y[0:n] = X[0:n] < 0 ? 0 : X[0:n] (a NaN stays a NaN, as torch.relu), n % 8 == 0 (the decoder's MLPs; omg_gemm has no ReLU
 *   epilogue).  Y may be X.
 * ---------------------------------------------------------------------- */
int omg_attn_small(int dtype, int B, int heads, int head_dim, int Nq, int Nk,
                   const void* Q, int64_t ldq, int64_t q_bstride, const void* K, int64_t ldk, int64_t k_bstride,
                   const void* V, int64_t ldv, int64_t v_bstride, float scale,
                   void* O, int64_t ldo, int64_t o_bstride, void* stream);
int omg_convt2x2_ln_gelu(int dtype, const void* G, int64_t ldg, int B, int H, int W, int Cout, const void* bias,
                         const void* ln_gamma, const void* ln_beta, float eps, int act, void* Y, void* stream);
int omg_sam_mask_logits(int dtype, const void* hyper, const void* up, int B, int M, int64_t P, int C,
                        float* logits, void* stream);
int omg_sam_postprocess(const float* low, int N, int Hl, int Wl, int image_size, int in_h, int in_w,
                        int out_h, int out_w, float threshold, int out_u8, void* out, void* stream);
int omg_relu(int dtype, const void* X, void* Y, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * SAM's ViT image encoder (omg_amd/sam_vit.py: segment_anything's ImageEncoderViT).  Linear layers are omg_gemm, LayerNorms
 * omg_layernorm, the neck's 3x3 convolution omg_conv3x3_nhwc_act.
 * omg_attn_relpos: softmax attention per head with the decomposed relative-position bias, read straight from the fused QKV
 *   projection.  qkv [B H W][ld]: rows in image order, columns q | k | v, each heads * head_dim wide and head-major; out [B H W][ldo],
 *   head-major; ld, ldo multiples of 8, base pointers 16-byte aligned.  head_dim 64 | 80.
 *     score((qy, qx), (ky, kx)) = scale q.k + q.rel_h[qy - ky + Sh - 1] + q.rel_w[qx - kx + Sw - 1]
 *   with the bias terms on the UNSCALED q; rel_h [2 Sh - 1][head_dim], rel_w [2 Sw - 1][head_dim], contiguous, in the storage dtype.
 *   Scores, bias, softmax and P V are fp32 (16-bit MFMA operands); neither scores nor bias are written to memory.
 *   window == 0: the keys are all H W tokens of the sample, Sh = H, Sw = W.  Any H, W >= 1 up to what the bias tables may take of
 *     LDS: H + W <= 83, or W == 64 (a key tile is one image row) and H <= 335.
 *   window == S (S S <= 256): the grid is cut into ceil(H / S) x ceil(W / S) windows from the top left; a query attends to the S S
 *     positions of its own window with offsets taken inside the window (Sh = Sw = S).  A position beyond the H x W grid is a real key
 *     with k | v = pad_kv [2 heads head_dim] (null: zeros) — what zero padding after the norm gives: the k and v slices of the QKV
 *     bias.  Queries beyond the grid are not computed.
 *   B, H or W == 0: nothing to do.
 * omg_gelu_erf: Y[0:n] = erf GELU of X[0:n] (nn.GELU()), n % 8 == 0.  Y may be X.
 * ---------------------------------------------------------------------- */
int omg_attn_relpos(int dtype, int B, int H, int W, int heads, int head_dim, int window, const void* qkv, int64_t ld,
                    const void* rel_h, const void* rel_w, const void* pad_kv, float scale, void* out, int64_t ldo, void* stream);
int omg_gelu_erf(int dtype, const void* X, void* Y, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * The DPT-hybrid depth estimator (omg_amd/dpt.py: transformers' DPTForDepthEstimation for dpt-hybrid-midas, the network behind the
 * "Depth" spatial condition) and the tail of the demos' get_depth.  Linear layers and 1x1 convolutions are omg_gemm, LayerNorms
 * omg_layernorm, attention omg_attn_fwd, the MLP's activation omg_gelu_erf.  NHWC fp16 / bf16, fp32 accumulation and statistics,
 * one rounding at the store; deterministic, and a sample's result does not depend on the batch it is in.
 * TF-"SAME" padding at stride 2 (BiT): output size ceil(n / 2), total padding max((out - 1) 2 + k - n, 0), its smaller half in
 *   front and the rest behind.
 * omg_conv3x3_nhwc_ex: omg_conv3x3_nhwc_act's kernel with more of an epilogue.  act: 0 | 1 (tanh GELU) | 2 (ReLU).  flags bit 0: ReLU of
 *   the INPUT as it is loaded (the residual, if any, is read as it is stored); bit 1: at stride 2 the SAME origin instead of padding 1
 *   (padding in front: 0 for an even size, 1 for an odd one, per axis).  Output size (Hin - 1) / stride + 1 either way.
 * omg_dpt_stem_conv: Y[B, ceil(H/2), ceil(W/2), Cout] NHWC = conv7x7 stride 2, SAME, of the NCHW pixel values X [B, 3, H, W] (in_dtype:
 *   OMG_F32 or the storage dtype; rounded to the storage dtype as they are loaded).  Wp [Cout][148] in the storage dtype:
 *   k = (ky 7 + kx) 3 + c, the last element zero.  No bias.  Cout % 32 == 0, Cout <= 128.
 * omg_groupnorm_res_act: Y = relu?(GroupNorm(X) gamma + beta [+ residual]) over NHWC X [B, HW, C]; the statistics are omg_groupnorm's
 *   (same kernels, same workspace: omg_groupnorm_ws_floats); residual [B, HW, C] may be NULL; relu 0 | 1.  Y may be X.
 * omg_maxpool3x3s2_nhwc: 3x3 stride-2 max-pool under the SAME rule, padded with the VALUE 0 (which takes part in the maximum, as
 *   BitMaxPool2d pads before it pools) -> [B, ceil(H/2), ceil(W/2), C].  C % 8 == 0.
 * omg_upsample2x_bilinear_nhwc: Y [B, 2H, 2W, C] = bilinear resize, align_corners = True, as torch.nn.functional.interpolate computes
 *   it in fp32.  C % 8 == 0.
 * omg_rowdot_f32: Y[m] (fp32) = relu?(sum_c X[m][c] w[c] + bias[0]) for rows of ldx elements; w [C] and bias [1] (may be NULL) in the
 *   storage dtype.  C % 8 == 0.  The 32 -> 1 projection of the depth head.
 * omg_depth_tail: depth [B, h, w] fp32 -> out [B, H, W, 3] uint8:
 *     r = bicubic resize (a = -0.75, align_corners = False, as torch.nn.functional.interpolate) of a sample to H x W, in fp32;
 *     out = trunc(clip((r - min r) / (max r - min r) * 255, 0, 255)), the same byte three times.
 *   Minimum and maximum are those of the RESIZED map (bicubic overshoots).  Two launches: per-block minima / maxima into the
 *   workspace (omg_depth_tail_ws_floats floats), then a fold of them in every block and the resize again — r is never stored.
 *   A constant map (where the reference divides zero by zero) gives zeros: max r - min r <= 2^-20 max(|min r|, |max r|), the rounding
 *   noise the resize itself leaves on equal inputs, counts as no range.
 * ---------------------------------------------------------------------- */
int omg_conv3x3_nhwc_ex(int dtype, const void* X, int B, int Hin, int Win, int Cin, int Cout, int stride,
                        const void* Wt, const void* bias, int act, const void* residual, int flags, void* Y, void* stream);
int omg_dpt_stem_conv(int in_dtype, int dtype, const void* X, int B, int H, int W, int Cout, const void* Wp, void* Y, void* stream);
int omg_groupnorm_res_act(int dtype, const void* X, int B, int HW, int C, int groups, float eps, const void* gamma, const void* beta,
                          const void* residual, int relu, float* workspace, void* Y, void* stream);
int omg_maxpool3x3s2_nhwc(int dtype, const void* X, int B, int H, int W, int C, void* Y, void* stream);
int omg_upsample2x_bilinear_nhwc(int dtype, const void* X, int B, int H, int W, int C, void* Y, void* stream);
int omg_rowdot_f32(int dtype, const void* X, int64_t ldx, int64_t M, int C, const void* w, const void* bias, int relu, float* Y,
                   void* stream);
int64_t omg_depth_tail_ws_floats(int B, int H, int W);
int omg_depth_tail(const float* depth, int B, int h, int w, int H, int W, float* workspace, void* out, void* stream);

/* ------------------------------------------------------------------------
 * The Swin backbone (omg_amd/swin.py: transformers' SwinBackbone, the image backbone of GroundingDINO).  Linear layers are omg_gemm,
 * LayerNorms omg_layernorm, the MLP's activation omg_gelu_erf.
 * omg_attn_swin: (shifted-)window softmax attention per head, head_dim 32, read straight from the fused QKV projection.  qkv
 *   [B H W][ld]: rows in image order, columns q | k | v, each heads * 32 wide and head-major; out [B H W][ldo], head-major; ld, ldo
 *   multiples of 8, base pointers 16-byte aligned.  window S = 7 | 12, shift 0 | S / 2, any heads >= 1, any H, W >= 1 (grids smaller
 *   than the window included: the window is never clamped, as SwinBackbone runs its encoder with always_partition).
 *   The grid is padded at the bottom and right to (Hp, Wp), multiples of S, rolled by -shift on both axes, and cut into S x S windows
 *   from the top left; none of that is materialised: position (ry, rx) of the rolled grid is position ((ry + shift) mod Hp,
 *   (rx + shift) mod Wp) of the padded one.  A query attends to the S S positions of its window:
 *     score(q, k) = scale q.k + table[(qiy - kiy + S - 1) (2 S - 1) + (qix - kix + S - 1)][head]  (+ -100 if region(q) != region(k))
 *   with (iy, ix) the position inside the window; table [(2 S - 1)^2][heads] is the checkpoint's relative_position_bias_table in the
 *   storage dtype.  region (shift > 0 only) = 3 band(ry, Hp) + band(rx, Wp), band(c, n) = [0, n - S) | [n - S, n - shift) |
 *   [n - shift, n): the additive mask of SwinLayer.get_attn_mask, not an exclusion.
 *   A position beyond the H x W grid is a real key, shifted or not, with k | v = pad_kv [2 heads 32] (null: zeros) — what zero
 *   padding after the norm gives: the k and v slices of the QKV bias.  Queries beyond the grid are not computed, their rows not
 *   written; out columns beyond heads * 32 are not written.  The keys that only pad 49 to the MFMA tile are excluded exactly.
 *   Scores, bias, mask, softmax and P V are fp32 (16-bit MFMA operands); a window's softmax is one pass over registers.  The
 *   reduction order inside a (window, head) is fixed: results do not depend on the batch or on other windows.
 * omg_swin_patch_embed: Y [B ceil(H/4) ceil(W/4)][ldy] = the 4 x 4 stride-4 patches of the NCHW pixel values X [B, 3, H, W] (in_dtype:
 *   OMG_F32 or the storage dtype), zero beyond the image; column k = (c 4 + ky) 4 + kx, the order of projection.weight.reshape(C, 48);
 *   columns 48 .. ldy - 1 are written as zeros.  ldy % 8 == 0, ldy >= 48.
 * omg_swin_merge_ln: Y [B ceil(H/2) ceil(W/2)][4 C] = LayerNorm over 4 C (fp32 statistics, two passes over registers) of the 2 x 2
 *   neighbourhoods of X [B, H, W, C], channel blocks (dy, dx) = (0,0), (1,0), (0,1), (1,1); a position beyond an odd H or W is zeros
 *   BEFORE the norm.  gamma, beta [4 C].  C % 8 == 0, C <= 1024.
 * ---------------------------------------------------------------------- */
int omg_attn_swin(int dtype, int B, int H, int W, int heads, int window, int shift, const void* qkv, int64_t ld,
                  const void* table, const void* pad_kv, float scale, void* out, int64_t ldo, void* stream);
int omg_swin_patch_embed(int in_dtype, int dtype, const void* X, int B, int H, int W, void* Y, int64_t ldy, void* stream);
int omg_swin_merge_ln(int dtype, const void* X, int B, int H, int W, int C, const void* gamma, const void* beta, float eps,
                      void* Y, void* stream);

/* ------------------------------------------------------------------------
 * GroundingDINO's feature enhancer (omg_amd/gdino.py: transformers' GroundingDinoEncoder and the neck in front of it).  Linear layers
 * and the neck's 1x1 convolutions are omg_gemm, LayerNorms omg_layernorm, the neck's GroupNorm omg_groupnorm_res_act, the extra
 * level omg_conv3x3_nhwc_act at stride 2, the MLPs' activation omg_relu.  Storage fp16 / bf16, arithmetic fp32, one rounding at the
 * store; no atomics; every reduction order is fixed by the sample's own sizes, so a sample's result does not depend on the batch it is
 * in and a graph replay equals the eager call.  Byte masks: 1 (non-zero) = valid / attend, 0 = padded / excluded, everywhere.
 *
 * omg_msdeform_attn: what GroundingDinoMultiscaleDeformableAttention.forward does between its Linear layers.
 *   value [B N][ldv]: the rows of value_proj, head-major, heads x 32; mask [B N] or NULL: a row whose byte is 0 reads as zeros (the
 *     library's masked_fill of the value, NOT a score mask).
 *   ow [B Nq][ldow]: the fused rows of sampling_offsets | attention_weights: heads L 4 2 offsets ordered (head, level, point, xy), then
 *     heads L 4 logits ordered (head, level point).  ref [B Nq L 2] fp32, (x, y) in [0, 1] units of each sampled level.
 *   H[l], W[l], start[l]: level l is rows start[l] .. start[l] + H[l] W[l] - 1 of a sample, row-major.
 *   Per (query, head): a = softmax over the L 4 logits; loc = ref + off / (W_l, H_l); pixel x = loc_x W_l - 0.5 (computed as
 *     ref_x W_l + off_x - 0.5), y alike: bilinear, align_corners = False, a corner outside the level contributes 0;
 *     out [B Nq][ldo] (head-major) = sum over level, point, corner of a w_corner value, in that order, fp32.
 *   head_dim 32, points 4, 1 <= L <= 4: anything else is refused.  Row strides multiples of 8, base pointers 16-byte aligned.  Value
 *     rows are taken to be finite (a corner of weight 0 is still read, from a clamped address).  out columns beyond heads 32 are not
 *     written.  B or Nq == 0: nothing to do.
 *
 * omg_attn_bi_vision / omg_attn_bi_text: the two halves of GroundingDinoBiMultiHeadAttention, head_dim 256, read from the fused
 *   projection rows vis [B N][ld_vis] = vision q | vision v and txt [B T][ld_txt] = text k | text v (each heads 256 wide, head-major;
 *   samples vis_bstride / txt_bstride elements apart).  T <= 256.  scale is the library's `scale` on q, applied to the fp32 score in
 *   the exponent.
 *     vision: out [B N][ldo] = softmax_t(scale q_n . k_t) v_text, text_mask [B T] or NULL excludes padded text keys.
 *     text:   out [B T][ldo] = softmax_n(scale q_n . k_t) v_vision over ALL N image keys, vision_mask [B N] or NULL excludes padded
 *             image keys.  The keys are cut into nchunks = ceil(N / chunk) chunks, chunk = omg_attn_bi_text_chunk(N) (a function of
 *             N alone: 64 up to N = 4096, then the multiple of 64 that gives at most 64 chunks); every chunk's maximum, sum and
 *             accumulator [T, 256] go to the workspace in fp32 (omg_attn_bi_text_ws_floats floats, 16-byte aligned) and a second
 *             launch folds them in ascending chunk order.  A chunk whose keys are all excluded folds in with weight 0.
 *   The library subtracts the global maximum (vision) or the row maximum (text) and clamps the scores to +- 50000 before its
 *   softmaxes.  The shifts cancel in a softmax; the CLAMP IS NOT REPRODUCED: results differ from the library's only where the scores
 *   of one softmax spread by more than 5e4.  A row whose keys are ALL excluded is NaN in the library and UNDEFINED (finite) here; the
 *   model never makes one.
 *
 * omg_attn_masked: O [B Nq][ldo] = softmax(scale Q K^T under mask) V per head, head_dim 64, Nq, Nk <= 256, mask [B Nq Nk] bytes (the
 *   same for every head) or NULL: the text enhancer's self-attention under the phrase block mask.  Q, K, V, O: rows of ld* elements,
 *   samples *_bstride elements apart, head h at column 64 h.  A fully excluded row is undefined (finite).
 *
 * All three attentions: scores, softmax and P V in fp32 on 16-bit MFMA operands; the probabilities are rounded to the storage type
 * for the second product and summed AS ROUNDED; the keys run through LDS in tiles of 64 under an online softmax.
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t dtype;
  int32_t B, N, Nq;           /* value rows and query rows per sample                */
  int32_t heads, head_dim;    /* head_dim == 32                                       */
  int32_t L, points;          /* 1 <= L <= 4, points == 4                             */
  int32_t H[4], W[4], start[4];
  const void* value; int64_t ldv;
  const uint8_t* mask;        /* [B, N] or NULL                                       */
  const void* ow; int64_t ldow;
  const float* ref;           /* [B, Nq, L, 2]                                        */
  void* out; int64_t ldo;
} omg_msdeform_args;

int omg_msdeform_attn(const omg_msdeform_args* a, void* stream);
int omg_attn_bi_vision(int dtype, int B, int heads, int N, int T, const void* vis, int64_t ld_vis, int64_t vis_bstride,
                       const void* txt, int64_t ld_txt, int64_t txt_bstride, const uint8_t* text_mask, float scale,
                       void* out, int64_t ldo, int64_t o_bstride, void* stream);
int omg_attn_bi_text_chunk(int N);
int64_t omg_attn_bi_text_ws_floats(int B, int heads, int T, int N);
int omg_attn_bi_text(int dtype, int B, int heads, int N, int T, const void* vis, int64_t ld_vis, int64_t vis_bstride,
                     const void* txt, int64_t ld_txt, int64_t txt_bstride, const uint8_t* vision_mask, float scale,
                     float* workspace, void* out, int64_t ldo, int64_t o_bstride, void* stream);
int omg_attn_masked(int dtype, int B, int heads, int Nq, int Nk, const void* Q, int64_t ldq, int64_t q_bstride,
                    const void* K, int64_t ldk, int64_t k_bstride, const void* V, int64_t ldv, int64_t v_bstride,
                    const uint8_t* mask, float scale, void* O, int64_t ldo, int64_t o_bstride, void* stream);

/* ------------------------------------------------------------------------
 * GroundingDINO's query selection, decoder and heads (omg_amd/gdino_decoder.py: transformers' GroundingDinoModel.forward from "prepare
 * decoder inputs" on, GroundingDinoDecoder and the head loop of GroundingDinoForObjectDetection).  The rules of the block above hold.
 *
 * omg_attn_hd32: O [B Nq][ldo] = softmax(scale Q K^T under key_mask) V per head at head_dim 32, any Nq, Nk >= 1; key_mask [B Nk] bytes
 *   (the same for every query and head) or NULL.  The decoder's self-attention (no mask) and its text cross-attention (the padded-token
 *   mask; the library adds finfo.min to padded keys, which is the same thing except for an all-excluded row: undefined and finite
 *   here).  Operands as omg_attn_masked: rows of ld* elements, samples *_bstride apart, head h at column 32 h — a column slice of a fused
 *   projection buffer is an operand.  The tiled kernel of the block above at D = 32: one 16x16x32 MFMA step per 16-key tile.
 *
 * omg_msdeform_attn_box: omg_msdeform_attn with box reference points, ref [B Nq L 4] fp32 (cx, cy, w, h) per sampled level (16-byte
 *   aligned): loc = (cx, cy) + off / 4 (w, h) 0.5; pixel x = loc_x W_l - 0.5, FORMED AS fma(cx, W_l, fma(off_x, s, -0.5)) with
 *   s = w (W_l / 8) rounded once (W_l / 8 is exact), y alike with h and H_l.  Everything else — lanes, taps, summation order, the value
 *   mask, the clamp of far-out coordinates, the checks — is omg_msdeform_attn's.
 *
 * omg_gdino_contrastive: GroundingDinoContrastiveEmbedding.  S[b, n, t] = X[b, n, :] . Y[b, t, :] over 256 channels, X [B N][ldx],
 *   Y [B T][ldy], 1 <= T <= max_text_len <= 256 (a multiple of 4), text_mask [B T] bytes.  16-bit MFMA operands, fp32 accumulation,
 *   stored without a rounding to 16 bits.  logits [B, N, max_text_len] fp32 or NULL: masked tokens and columns T .. max_text_len - 1
 *   hold -inf.  rowmax [B, N] fp32 or NULL: bitwise the maximum of what logits holds.  At least one of the two.
 *
 * omg_gdino_ref_step: the reference bookkeeping of one decoder layer, one launch.  rows = B Q.
 *   base  = logit_in [rows 4] (may hold +inf) if given, else torch.special.logit(ref_in [rows 4], eps = 1e-5); exactly one of the two.
 *   Hd [rows][ldh] (the box head's second hidden state, 256 wide) with W3 [4, 256], b3 [4], or NULL:
 *     Hd given:  ref_out = sigmoid(W3 Hd + b3 + base), the product in fp32, never rounded to 16 bits;
 *     Hd NULL:   ref_out = ref_in as it is (the step in front of layer 0), or sigmoid(logit_in).
 *   ref_input [rows L 4] fp32 or NULL = ref_out times (vx, vy, vx, vy) of valid_ratios [B L 2] per level.
 *   emb [rows][lde] (storage type, 512 wide) or NULL = encode_sinusoidal_position_embedding(ref_input[:, 0, :], 128): blocks y, x, w, h.
 * ---------------------------------------------------------------------- */
int omg_attn_hd32(int dtype, int B, int heads, int Nq, int Nk, const void* Q, int64_t ldq, int64_t q_bstride,
                  const void* K, int64_t ldk, int64_t k_bstride, const void* V, int64_t ldv, int64_t v_bstride,
                  const uint8_t* key_mask, float scale, void* O, int64_t ldo, int64_t o_bstride, void* stream);
int omg_msdeform_attn_box(const omg_msdeform_args* a, void* stream);
int omg_gdino_contrastive(int dtype, int B, int N, int T, int max_text_len, const void* X, int64_t ldx, const void* Y, int64_t ldy,
                          const uint8_t* text_mask, float* logits, float* rowmax, void* stream);
int omg_gdino_ref_step(int dtype, int B, int Q, int L, const float* ref_in, const float* logit_in, const float* valid_ratios,
                       const void* Hd, int64_t ldh, const void* W3, const void* b3, float* ref_out, float* ref_input,
                       void* emb, int64_t lde, void* stream);

/* ------------------------------------------------------------------------
 * GroundingDINO's BERT text encoder (omg_amd/bert.py: transformers' BertModel without its pooler).  Attention is omg_attn_masked on
 * column slices of the fused q | k | v rows, LayerNorms omg_layernorm.  Storage fp16 / bf16, arithmetic fp32, one rounding at the store;
 * no atomics, no workspace; every reduction order is fixed by the operand's own sizes.
 *
 * omg_gemm_skinny: C[M, N] = epi(A[M, K] W[N, K]^T) for FEW rows (a caption is 6 to 30 tokens): the launch is a stream of W, so the
 *   work is cut along N and never along M.
 *   A [M][lda], W [N][ldw] (torch Linear layout), C [M][ldc], residual [M][ldr]: row strides in ELEMENTS, multiples of 8 and at least
 *     the row's length, base pointers 16-byte aligned — a column slice of a wider buffer is an operand.  K % 8 == 0, N % 8 == 0 (the
 *     rules of omg_gemm), any M >= 1.
 *   epi, in this order: + bias [N] (or NULL); gelu = 1: the erf GELU of omg_gelu_erf (gelu.h, not a tanh form); + residual (or NULL),
 *     added AFTER the activation.  Products on the 16-bit MFMA (16x16x32), sums and the epilogue in fp32, ONE rounding at the store.
 *   Work split: a workgroup owns 8 columns of N (16 from N = 2048 on) over the WHOLE of K, so every workgroup streams its own rows of
 *     W exactly once and nothing is reduced across workgroups: no atomics, no workspace, no second launch.  K is cut into steps of 64
 *     elements; wave w of the workgroup's four takes the steps w, w + 4, w + 8, ... in ascending order and the four fp32 partial tiles
 *     are added through LDS in ascending wave order.  The split is a function of K alone.  Up to 64 rows share one pass over the
 *     workgroup's weights; further rows are a second grid dimension (their weights come from L2).
 *   Invariance: the bits of row r of C depend on row r of A, on W and on row r of the epilogue operands — not on M, not on r's position
 *     in the call, not on what other rows hold (Inf and NaN included), not on the column slice width.
 *   Nothing outside an operand is read: a K tail (a multiple of 8, not of 64), an N tail narrower than a slice and the rows that pad M
 *     to the MFMA tile are read from a clamped address inside the operand and replaced by zeros in registers.
 *   Refused with a message: dtype, NULL A / W / C, M, N or K < 1, K or N not a multiple of 8, a stride that is not a multiple of 8 or
 *     shorter than its row, a misaligned base, gelu other than 0 / 1, M beyond 64 * 65535.
 *
 * omg_bert_embed_ln: BertEmbeddings.forward for inference, one launch.  Per token t of M:
 *     Y[t] = LayerNorm(word[input_ids[t]] + type[token_type_ids[t]] + pos[position_ids[t]]) * gamma + beta
 *   the sum formed in that order in fp32, two-pass fp32 statistics over the row in registers (omg_layernorm's), eps a float (BERT's is
 *   1e-12), one rounding to the storage type.  The ids are the int64 tensors torch holds, read on the device: no cast pass, no host
 *   synchronisation.  word [n_word][C], type [n_type][C], pos [n_pos][C] contiguous, Y [M][ldy].
 *   AN ID OUTSIDE ITS TABLE IS CLAMPED INTO IT (below 0 -> row 0, at or above the size -> the last row): a kernel cannot report it
 *   and must not read outside the table.  C % 8 == 0, 8 <= C <= 4096 (one wave holds a row); beyond that the call is refused.
 * ---------------------------------------------------------------------- */
int omg_gemm_skinny(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias,
                    int gelu, const void* residual, int64_t ldr, void* C, int64_t ldc, void* stream);
int omg_bert_embed_ln(int dtype, int M, int C, const int64_t* input_ids, const int64_t* token_type_ids, const int64_t* position_ids,
                      const void* word, int n_word, const void* type, int n_type, const void* pos, int n_pos,
                      const void* gamma, const void* beta, float eps, void* Y, int64_t ldy, void* stream);

/* ------------------------------------------------------------------------
 * Pillow's 8-bit resize on the device, and what a preprocessor does behind it (omg_amd/image_prep.py).  Image.resize(size, resample) on
 * an RGB image is two passes over tables that depend on the sizes alone (image_prep.resize_tables, float64 on the host, uploaded once):
 *   bounds [out][2] int32: first input index and number of taps n of an output index; coeffs [out][ksize] int32: 22-bit fixed point.
 *   a pass:  out = clip((2^21 + sum_{t < n} in[first + t] * coeff[t]) >> 22, 0, 255)  in 32-bit integers, per channel.
 * The kernels read the tables and know no filter: BILINEAR and BICUBIC cost the same.  A window is clamped into its axis, so a table
 * that is not resize_tables' own cannot make a kernel read outside the image.  No atomics, no workspace; the result is a function of
 * the input and the tables alone, bit for bit what Pillow computes.
 *
 * omg_image_resize_h: the horizontal pass, uint8 in [B][H][W][3] -> uint8 out [B][H][OW][3], both contiguous; bounds / coeffs of W -> OW.
 *   A wave stages the segment of its row that 64 outputs read in LDS through aligned dword loads (nothing behind the tensor is read:
 *   its last partial dword goes byte by byte); a segment beyond 4 KiB or an input that is not 4-byte aligned is read from global memory.
 * omg_image_resize_v: the vertical pass, uint8 in [B][H][W][3] -> OH rows; bounds / coeffs of H -> OH, or bounds NULL: OH == H, the
 *   identity (the epilogue alone).  The epilogue:
 *     lut NULL:  uint8 out [B][OH][W][3];
 *     lut given: out [B][3][Hpad][Wpad] of out_dtype (OMG_F16 / OMG_BF16 / OMG_F32), out[b][c][y][x] = lut[c][value] with lut [3][256]
 *                of out_dtype, and 0 for y >= OH or x >= W (Hpad >= OH, Wpad >= W): normalise, pad, permute and cast in the store.
 * Refused with a message: NULL operands, sizes below 1, misaligned tables, a pad smaller than the image, an unknown out_dtype,
 *   B H beyond 4 * 65535 rows (h), B beyond 65535 or more than 4 * 65535 output rows (v).
 * ---------------------------------------------------------------------- */
int omg_image_resize_h(int B, int H, int W, int OW, const uint8_t* in, const int32_t* bounds, const int32_t* coeffs, int ksize,
                       uint8_t* out, void* stream);
int omg_image_resize_v(int B, int H, int W, int OH, const uint8_t* in, const int32_t* bounds, const int32_t* coeffs, int ksize,
                       int out_dtype, const void* lut, int Hpad, int Wpad, void* out, void* stream);

/* ------------------------------------------------------------------------
 * Building one weight slot of a LoRA bank (omg_amd/lora.py, LoraBank.build): the merge of up to OMG_LORA_MAX_TERMS adapter terms into the
 * 16-bit base weight W [N][K] (a Linear's [out][in], a convolution's packed [out][tap * Cin + cin]), all arithmetic in fp32:
 *
 *     out[n][k] = round16( W[n][k] * (1 + sum_t (gain_t[n] - 1)) + sum_t gain_t[n] * s_t * D_t[n][k] )        gain_t == 1 where NULL
 *
 * A term's dense delta D_t never goes to memory; it is formed per 32 x 64 tile in registers from the term's small fp32 factors (the sum
 * of the terms crosses LDS once, to meet W in row-major order):
 *   OMG_LORA_PLAIN  D = f0 [N][r] . f1 [r][K]                                       (lora_up . lora_down)
 *   OMG_LORA_HADA   D = (f0 [N][r] . f1 [r][K]) * (f2 [N][r2] . f3 [r2][K])          elementwise (LoHa)
 *   OMG_LORA_KRON   D[ia * c + ic][tap * (b * d) + ib * d + id] = f0[ia][ib] * f1[ic][tap][id]     f0 [a][b], f1 [c][taps][d] (LoKr)
 *                   with a * c == N and taps * b * d == K.
 * The products of PLAIN and HADA run on v_mfma_f32_32x32x2_f32: exact fp32 products, one fmaf chain per element over the rank in one
 * fixed order (ranks are padded to a multiple of eight with zero products).  An element's value depends on its own row and column only — not
 * on N, on its tile or on the other rows.  W is read once, out written once, one rounding at the store; out may be W itself.
 *
 * omg_lora_rownorm: norm[n] = sqrt(sum_k (W[n][k] + s * D[n][k])^2) of ONE term (DoRA's weight norm; the term's gain is ignored).  A
 *   workgroup owns 32 rows: four waves take the 64-column tiles round robin, a lane adds its squares in ascending column order, the
 *   partial sums are folded in a fixed order.  No atomics, no workspace: the result is a function of the operands alone.
 * Refused with a message: dtype, NULL operands, N < 1, K < 8 or K % 8 != 0, more than OMG_LORA_MAX_TERMS terms, an unknown kind,
 *   r < 1, a KRON whose dims do not multiply to N and K, a misaligned W / out.
 * ---------------------------------------------------------------------- */
enum { OMG_LORA_PLAIN = 0, OMG_LORA_HADA = 1, OMG_LORA_KRON = 2 };
#define OMG_LORA_MAX_TERMS 4
typedef struct {
  int32_t kind;            /* OMG_LORA_PLAIN / HADA / KRON */
  int32_t r, r2;           /* PLAIN: r; HADA: ranks of the first and the second product; KRON: unused */
  int32_t a, b, c, d, taps; /* KRON only */
  float s;                 /* the whole scaling of the term */
  int32_t pad_;
  const float* f0;
  const float* f1;
  const float* f2;
  const float* f3;
  const float* gain;       /* [N] or NULL */
} omg_lora_term;
typedef struct {
  int32_t dtype, N, K, n_terms;
  const void* W;           /* [N][K] of dtype */
  void* out;               /* [N][K] of dtype: one slot of the stack */
  omg_lora_term terms[OMG_LORA_MAX_TERMS];
} omg_lora_merge_args;
int omg_lora_rownorm(int dtype, int N, int K, const void* W, const omg_lora_term* term, float* norm, void* stream);
int omg_lora_merge(const omg_lora_merge_args* a, void* stream);

/* ------------------------------------------------------------------------
 * The demos' Canny edge condition, cv2.Canny(image, threshold1, threshold2) at apertureSize 3 and L2gradient False, on the device
 * (omg_amd/canny.py: the arithmetic as a numpy model, written from OpenCV's published algorithm).  Integers throughout; every result is a
 * function of its input alone, whatever order the workgroups run in.
 *
 * omg_canny_nms: uint8 image [B][H][W][C] (C 1 or 3, contiguous, any byte alignment) -> uint8 state [B][H][W], one launch:
 *     dx, dy  3x3 Sobel per channel on the replicated border; mag = |dx| + |dy|; with C = 3 the channel of the largest mag (the lowest on a tie);
 *     mag counts as 0 outside the image; a pixel with mag > low is kept when it beats its two neighbours along the gradient's sector
 *     (|dy| 2^15 < |dx| 13573: left (>) and right (>=); |dy| 2^15 > |dx| 79109: up (>) and down (>=); else the diagonal pair, both >);
 *     state = 0 not kept, 1 kept and mag <= high, 2 kept and mag > high.
 *   A workgroup owns 64 x 16 pixels and stages their source bytes with a two-pixel halo in LDS through aligned dword loads (nothing
 *   outside the tensor is read: its first and last partial dwords go byte by byte); gradients and magnitudes never go to memory.
 * omg_canny_hysteresis: state [B][H][W] -> edges: set where the state is not 0 and the pixel's 8-connected component of non-zero states
 *   holds a state >= 2.  Union-find over pixel indices in four launches (three when the image is one tile), the same for any data; no
 *   host synchronisation, no copy, no kernel waits for another workgroup.  workspace: omg_canny_hysteresis_ws_bytes bytes, 4-byte
 *   aligned, written before it is read (nothing to initialise).  out_form:
 *     0  uint8 [B][H][W]      0 / 255
 *     1  uint8 [B][H][W][3]   the same byte three times (get_cannyedge's image)
 *     2  [B][3][H][W] of out_dtype (OMG_F16 / OMG_BF16 / OMG_F32)   0 / 1, what a ControlNet takes (image / 255, planar)
 * Refused with a message: NULL operands, C not 1 or 3, sizes below 1, B > 65535, H > 16 * 65535, B H W >= 2^29, low < 0 or high < low,
 *   an unknown out_form / out_dtype, a misaligned workspace or planar output.
 * ---------------------------------------------------------------------- */
int omg_canny_nms(int B, int H, int W, int C, const uint8_t* image, int low, int high, uint8_t* state, void* stream);
int64_t omg_canny_hysteresis_ws_bytes(int B, int H, int W);
int omg_canny_hysteresis(int B, int H, int W, const uint8_t* state, void* workspace, int out_form, int out_dtype, void* out, void* stream);

/* ------------------------------------------------------------------------
 * TOOLS AND TESTS ONLY — not part of the product path and no promise of stability.  Process-wide switches
 * (not thread-safe; set them while no call is in flight) and host-side queries of tools/ and tests/.  omg_debug_gemm_offset_limit
 * is declared above, with the GEMM family it describes.
 *   omg_debug_set_glds: 0 = the register-staged build of the 128x128 GEMM kernel instead of its LDS-DMA one; anything else = default.
 *   omg_debug_set_gemm_variant: bits 0-7 force one GEMM tile configuration (0 = the cost model chooses), the bits above are debug bits
 *     of the chosen kernel (tools/).  omg_debug_choose_variant: host-only, the configuration the cost model picks for (rows per group,
 *     groups, N, conv bit 0: a convolution, bit 1: a GEGLU epilogue).
 *   omg_debug_read_ts: copies the block timestamps that debug bit 16 of the large-tile GEMM kernels leaves (6 per block, at most 8192
 *     blocks) to the HOST buffer `out`; returns the hipError_t of the copy.
 *   omg_debug_set_mx8_split: the MX-fp8 GEMM's DMA split | debug bits << 8.
 *   omg_debug_set_attn_variant: bits 0-7 force one attention kernel (0 = the heuristic), the bits above are debug bits.
 * ---------------------------------------------------------------------- */
void omg_debug_set_glds(int on);
void omg_debug_set_gemm_variant(int v);
int omg_debug_choose_variant(int mrows, int groups, int N, int conv);
int omg_debug_read_ts(long long* out, int blocks);
void omg_debug_set_mx8_split(int d1);
void omg_debug_set_attn_variant(int v);

#ifdef __cplusplus
}
#endif
#endif /* OMG_HIP_H */
