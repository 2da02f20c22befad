/*
 * mudiff_hip.h - C ABI of libmudiff_hip.so: the MI355X (gfx950) kernels behind MU-Diff's
 * dual-generator reverse-diffusion sampling path.
 *
 * The reference has no FFI for this path except two pybind functions (utils/op/upfirdn2d.cpp:20-31,
 * utils/op/fused_bias_act.cpp:18-28); everything else is torch ops called from Python.  The entry
 * points below are what a binding for the path binds instead; each one names the reference code it
 * replaces (paths relative to the reference checkout).  Plain pointers and sizes only - no torch
 * types.  All pointers are DEVICE pointers unless a parameter says "host".  Every call enqueues on
 * `stream` (a hipStream_t passed as void*; NULL = the default stream), allocates nothing and never
 * synchronises, so a caller may capture any sequence of calls into a hipGraph.
 *
 * Activation layout: NHWC fp32, described as a *view* (ptr, B, H, W, C, ld): element (b,y,x,c) lives
 * at ptr[((b*H + y)*W + x)*ld + c] with ld >= C, so a channel slice of a wider tensor (the
 * concatenations of the U-Net) is a view and never a copy.  With C == 1 (the generator inputs and
 * outputs) NHWC and the reference's NCHW coincide.
 *
 * Return value: 0 on success, a MUD_ERR_* code otherwise; mud_last_error() gives the text.
 */
#ifndef MUDIFF_HIP_H
#define MUDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUD_OK 0
#define MUD_ERR_ARG 1      /* bad shape / alignment / null pointer                 */
#define MUD_ERR_LAUNCH 2   /* hipGetLastError() after a launch reported a failure  */
#define MUD_ERR_UNSUPPORTED 3

#define MUD_ACT_NONE 0
#define MUD_ACT_SIGMOID 1
#define MUD_ACT_TANH 2
#define MUD_ACT_SILU 3
#define MUD_ACT_LRELU 4      /* LeakyReLU(0.2): the critic's activation (backbones/discriminator.py:178) */

#define MUD_PRO_NONE 0         /* A operand used as stored                                   */
#define MUD_PRO_AFFINE 1       /* a[b,c]*x + s[b,c]            (GroupNorm, AttnBlockpp)      */
#define MUD_PRO_AFFINE_SILU 2  /* silu(a[b,c]*x + s[b,c])      (AdaGN + SiLU of the ResBlock) */
#define MUD_PRO_LRELU 3        /* lrelu_0.2(x), no affine      (DownConvBlock of the critic)  */
/* Not a value of pro_mode: the form of the 3x3 matrix-core kernel that a launch with pro_mode AFFINE_SILU and             */
/* mud_conv_args.in_up2 runs - FIR x2 up-sampling of silu(a*x + s), formed from the LOW-resolution x while it is staged. */
#define MUD_PRO_UP2_AFFINE_SILU 4
/* Not a value of pro_mode either: the form of the 3x3 matrix-core kernel that a launch with pro_mode NONE and mud_conv_args.in_s2d */
/* runs - the 2x2 space-to-depth view of x, gathered from the full-resolution tensor while it is staged.                          */
#define MUD_PRO_S2D 5

/* arithmetic plan of one mud_conv2d_mfma launch (mud_conv_args.prec); the weights must have been packed for the same plan */
#define MUD_PREC_16X3 0        /* every product as hi*hi + hi*lo + lo*hi on the 16-bit MFMA (fp16 pieces): ~2^-22 per product */
#define MUD_PREC_FP8X 1        /* hi*hi on the fp16 MFMA + both cross terms on the block-scaled e4m3 MFMA: ~2^-15 per product, */
                               /* 0.78x the matrix cycles; 3x3 launches that fill the chip (mud_conv2d_mfma_prec_supported)     */
#define MUD_PREC_16X1 2        /* ONE pass: fp16(a) * fp16(w) on the fp16 MFMA, fp32 accumulate: ~2^-11 per product, 1/3 of the */
                               /* 16x3 matrix cycles, hi-only weights at half the bytes.  Every 3x3 launch (no 1x1 form); the    */
                               /* accuracy class of autocast, NOT the parity plan (~1-2e-2 per sampling step from the reference)  */

int mud_version(void);
const char* mud_last_error(void);
/* "" for the shipped build; an experiment build (scripts/build_variants.py) reports the -D flags it was compiled with, so that a
 * library can always be asked what it is (mudiff_hip.load() refuses anything else unless MUDIFF_ALLOW_VARIANT=1). */
const char* mud_build_flags(void);
/* bytes of device workspace the calls below need at most for a given problem: see each call */

/* ---- L3: Gaussian posterior / forward diffusion (engine/test.py:126-177, engine/train.py:256-281)
 * out = 0.5*((c1[t]*x01 + c2[t]*xt) + (c1[t]*x02 + c2[t]*xt)) + (t != 0) * std[t] * noise
 * x02 == NULL gives the single-predictor sample_posterior (engine/test.py:126-147).
 * std[t] = exp(0.5*posterior_log_variance_clipped[t]) is a host-made table (engine/test.py:143,173).
 * The arithmetic is un-contracted fp32 mul/add in the reference's order: results are bit-identical
 * to the PyTorch-CPU path.  t is int64 [B]; indices are clamped to [0, ntab). */
int mud_posterior_sample(const float* x01, const float* x02, const float* xt, const float* noise,
                         const int64_t* t, const float* coef1, const float* coef2, const float* std_tab,
                         int ntab, float* out, int B, int64_t per_sample, void* stream);
/* out = a_tab[t+toff]*x + s_tab[t+toff]*noise   (q_sample: a_s_cum/sigmas_cum, toff 0;
 * second half of q_sample_pairs: a_s/sigmas, toff 1).  engine/train.py:256-281. */
int mud_q_sample(const float* x, const float* noise, const int64_t* t, int toff, const float* a_tab,
                 const float* s_tab, int ntab, float* out, int B, int64_t per_sample, void* stream);

/* ---- embeddings and the small dense path (backbones/layers.py:465-479, dense_layer.py:67-71,
 *      ncsnpp_generator_adagn_feat.py:44-49,271-277,301-305; layerspp.py:42,277) */
int mud_timestep_embedding(const int64_t* t, float* out, int B, int dim, float max_positions, void* stream);
int mud_pixel_norm(const float* z, float* out, int B, int K, void* stream);
/* out[b, n] = act_out( sum_k W[n,k] * act_in(in[b,k]) + bias[n] ),  W row-major [N,K] (nn.Linear). */
int mud_dense(const float* in, int ldi, const float* W, const float* bias, float* out, int ldo,
              int B, int K, int N, int act_in, int act_out, void* stream);

/* A chain of dense layers in one launch (one workgroup per sample):  h = [pixel_norm](x);  for l: h = W[l] h + b[l], with
 * `act` applied between layers (and after the last one iff act_last).  The z-mapping network (PixelNorm, dense(nz, z_emb),
 * SiLU, n_mlp x [dense, SiLU]; ncsnpp_generator_adagn_feat.py:44-49,271-277) is {pixel_norm=1, act=SILU, act_last=1}; the
 * timestep MLP (:301-305: Linear, SiLU, Linear) is {act=SILU, act_last=0}.  W[l]: [dims[l+1], dims[l]] row-major (nn.Linear). */
#define MUD_MLP_MAX_LAYERS 6
typedef struct mud_mlp_args {
  const float* x; int ldx; int B;
  int nlayers; int dims[MUD_MLP_MAX_LAYERS + 1];
  const float* W[MUD_MLP_MAX_LAYERS]; const float* b[MUD_MLP_MAX_LAYERS];
  int pixel_norm; int act; int act_last;
  float* out; int ldo;
  int maxdim;                                    /* filled in by the library */
} mud_mlp_args;
int mud_mlp_chain(const mud_mlp_args* a, void* stream);
/* n (<= 4) independent chains a[0..n) in one launch (the z-mapping network and the timestep MLP of a generator do not depend on  */
/* each other).                                                                                                                 */
int mud_mlp_chains(const mud_mlp_args* a, int n, void* stream);

/* ---- GroupNorm statistics -> per-(sample, channel) scale/shift for a consumer's prologue
 *      (torch native_group_norm as used by backbones/layerspp.py:37-65,103, eps 1e-6, biased var).
 * scale[b,c] = gamma[b,c] * rstd[b,g(c)],  shift[b,c] = beta[b,c] - mean[b,g(c)] * scale[b,c]
 * gamma/beta: NULL (=1/0), per channel (g_bstride 0) or per sample (g_bstride = row stride).
 * ws: device workspace of mud_gn_ws_bytes(B, HW, C, G) bytes. */
int64_t mud_gn_ws_bytes(int B, int64_t HW, int C, int G);
int mud_gn_scale_shift(const float* x, int B, int64_t HW, int C, int ld, int G, float eps,
                       const float* gamma, const float* beta, int64_t g_bstride,
                       float* scale, float* shift, int ld_ss, float* mean_rstd /* [B,G,2] or NULL */,
                       void* ws, void* stream);
/* Same result from per-channel (sum, sumsq) already accumulated by the producer's epilogue
 * (mud_conv_args.stats, mud_gate_mix): sums[(b*sums_ld + c)*2 + {0,1}], `count` = pixels per channel. */
int mud_gn_scale_shift_from_sums(const double* sums, int sums_ld, int B, int C, int G, double count, float eps,
                                 const float* gamma, const float* beta, int64_t g_bstride,
                                 float* scale, float* shift, int ld_ss, void* stream);
/* out[b,c] = mean over pixels (nn.AdaptiveAvgPool2d(1), layerspp.py:473,491). ws as above with G=C. */
int mud_channel_mean(const float* x, int B, int64_t HW, int C, int ld, float* out, int ldo, void* ws, void* stream);

/* ---- convolutions (torch F.conv2d call sites: layers.py:104-128, layerspp.py:275-285,399-408,
 *      ncsnpp_generator_adagn_feat.py:267,620-631; NIN einsum layers.py:502-505; the attention
 *      contractions layerspp.py:118-122) */
typedef struct mud_conv_args {
  const float* x;  int B, H, W, Cin, ldx;        /* input view                                      */
  const void* w;   int64_t w_bstride;            /* weights (format depends on the call); bytes     */
                                                 /* between per-sample weight sets, 0 = shared       */
  int ks, stride, pad;                           /* square kernel                                    */
  const float* pro_scale; const float* pro_shift; int pro_ld; int pro_mode;   /* [B,Cin] each        */
                                                 /* (mud_conv2d_mfma keeps them in LDS: Cin <= 1024  */
                                                 /* with pro_mode AFFINE / AFFINE_SILU)               */
  const float* bias;                             /* [Cout] or NULL                                   */
  const float* bias2; int bias2_ld;              /* [B,Cout] or NULL  (Dense_0(act(temb)))           */
  const float* res; int ldr;                     /* residual view [B,Ho,Wo,Cout] or NULL             */
  float out_scale; int act;                      /* v = act((acc+bias+bias2+res)*out_scale)          */
  const float* emul; int ld_emul;                /* optional: v *= emul[pixel, co]                   */
  const float* egate; int ld_egate;              /* optional gated mix (G2 feature fusion, ...feat.py */
  const float* eother; int ld_eother;            /* :779-788): v = egate*v + (1-egate)*eother         */
  float* out; int Cout, ldo;                     /* output view [B,Ho,Wo,Cout]                       */
  int sub2;                                      /* mud_conv2d_mfma, ks 3 only: compute the stride-1  */
                                                 /* pad-1 result and keep only odd (y,x) positions as */
                                                 /* out[(y-1)/2,(x-1)/2] == stride-2 pad-0 convolution */
                                                 /* of the input (the FIR'd pyramid, odd H and W)      */
  double* stats; int stats_ld;                   /* optional: per-(b, channel) running (sum, sum of   */
                                                 /* squares) of the STORED outputs, stats[(b*stats_ld */
                                                 /* + co)*2 + {0,1}] += ... (fp64 atomics); lets the   */
                                                 /* next GroupNorm skip its pass over the tensor       */
  int emul_cout;                                 /* `emul` applies to output channels < emul_cout only */
                                                 /* (0 = all): lets two convs that share their input   */
                                                 /* but differ in this epilogue run as one launch       */
  /* mud_conv2d_mfma only - GroupNorm finalisation folded into the prologue (pro_mode AFFINE / AFFINE_SILU): when gn_sums  */
  /* is set, pro_scale / pro_shift are ignored and every workgroup forms scale = gamma*rstd, shift = beta - mean*scale of   */
  /* its sample from the producer-accumulated per-channel (sum, sumsq) itself - the arithmetic of                           */
  /* mud_gn_scale_shift_from_sums, without its launch (layerspp.py:37-54 AdaptiveGroupNorm, :56-65 GroupNorm_Conv).         */
  const double* gn_sums; int gn_sums_ld;         /* gn_sums[(b*gn_sums_ld + c)*2 + {0,1}], c < Cin                           */
  int gn_G; float gn_eps; double gn_count;       /* groups (Cin % gn_G == 0), eps, pixels per channel                        */
  const float* gn_gamma; const float* gn_beta;   /* [Cin] (gn_bstride 0) or [B, .] rows gn_bstride floats apart, or NULL      */
  int64_t gn_bstride;
  /* mud_conv2d_mfma, ks 3 only - optional split-K workspace: when a launch would fill less than the chip (one slice at a   */
  /* time), the K chunks of a tile are dealt to several workgroups that write raw partial tiles here, and a second small     */
  /* launch adds them in a fixed order and applies the epilogue.  mud_conv2d_mfma_splitk_bytes() sizes it; NULL = never split. */
  void* splitk_ws; int64_t splitk_ws_bytes;
  /* optional arrival counters (splitk_ncounters of them, ZERO when handed over; every launch leaves them zero): with them the   */
  /* last workgroup to finish an output tile adds the slabs (same fixed order) and applies the epilogue, so a split convolution   */
  /* is one launch instead of two.  One array per stream: launches that may run concurrently must not share it.                   */
  unsigned* splitk_counters; int splitk_ncounters;
  /* mud_conv2d_mfma, ks 3, pro_mode AFFINE_SILU, plain epilogue - the residual block's 1x1 skip convolution of the RAW input     */
  /* (layerspp.py:320-321, x = Conv_2(x)) produced by the same launch: skip_out[pixel, co] = sum_ci x[pixel, ci] * skip_w + bias. */
  /* skip_w: mud_pack_weights(ks = 1) of the [Cout, Cin] matrix; x is then read from HBM once instead of twice.  Cin <= 512.      */
  const void* skip_w; const float* skip_bias; float* skip_out; int skip_ldo;
  /* mud_conv2d_mfma - arithmetic plan of this launch (MUD_PREC_*; 0 = the default) and, for MUD_PREC_FP8X, the power-of-two         */
  /* exponent the weights' e4m3 image was packed with (mud_pack_weights_prec: the largest e with max|w| * 2^e <= 448).               */
  int prec; int w_exp;
  /* mud_conv2d_mfma, ks 3, pro_mode AFFINE_SILU, no sub2 / skip_w, even H and W, a grid that is not split over K - the residual */
  /* up-sampled on load:                                                                                                        */
  /* with res_up2 != 0 `res` is the LOW-resolution view [B, H/2, W/2, Cout] and the residual of output (2i+a, 2j+b) is its x2 FIR */
  /* up-sampling by the separable 4x4 filter res_k (x) res_k (1-D taps, gain included; mud_fir_nhwc up = 2, pad (2, 1)):          */
  /* a = 0 takes rows i-1 (tap 3) and i (tap 1), a = 1 rows i (tap 2) and i+1 (tap 0), columns alike, outside the image = 0.     */
  /* Any other launch that sets it is refused (mud_conv2d_mfma_res_up2_supported tells beforehand); mud_conv2d_direct refuses it. */
  int res_up2; float res_k[4];
  /* mud_conv2d_mfma, ks 3, pro_mode AFFINE_SILU, no sub2 / skip_w / res_up2, even H and W, a grid that is not split over K - the  */
  /* INPUT up-sampled while it is staged (the up-sampling residual blocks' Conv_0): with in_up2 != 0 `x` is the LOW-resolution     */
  /* view [B, H/2, W/2, Cin] (H, W stay the output size; the folded GroupNorm's gn_count is that of the low-resolution tensor) and */
  /* the launch computes conv3x3(FIR x2 (silu(a*x + s))) - what mud_fir_nhwc(up = 2, pad (2, 1), the prologue) followed by a       */
  /* MUD_PRO_NONE launch computes, term for term - with the separable 4x4 filter in_k (x) in_k (1-D taps, gain included; rows and  */
  /* columns as for res_k).  Built for some tiles and plans only: mud_conv2d_mfma_in_up2_supported tells beforehand, any other      */
  /* launch that sets it is refused; mud_conv2d_direct refuses it.                                                                  */
  int in_up2; float in_k[4];
  /* mud_conv2d_mfma, ks 3, pro_mode NONE, no sub2 / skip_w / res_up2 / in_up2, a grid that is not split over K - the 2x2              */
  /* space-to-depth view of the input, gathered while it is staged (the input pyramid's FIR + stride-2 conv as ONE stride-1 launch:   */
  /* DESIGN 5.2c): with in_s2d != 0 `x` is the FULL-resolution tensor [B, 2H, 2W, Cin/4] with its own ldx, and H, W, Cin describe     */
  /* the folded view [B, H, W, Cin] the launch convolves: view channel (py*2 + px)*C + c, C = Cin/4, of view pixel (y, x) is element  */
  /* c of pixel (2y + py, 2x + px); the zero padding is the view's.  C must be a multiple of 16 (a 16-channel chunk never straddles    */
  /* two parities).  w_exp: the packed weights are W * 2^w_exp, and the launch takes the power of two back out of the accumulated sum   */
  /* before bias, residual and out_scale apply (exact; the composed weights' small taps stay normal fp16 numbers that way).            */
  /* Built for some tiles and plans only: mud_conv2d_mfma_in_s2d_supported tells beforehand, any other launch that    */
  /* sets it is refused; mud_conv2d_direct refuses it.                                                                                 */
  int in_s2d;
} mud_conv_args;

/* Exact fp32 direct convolution (FMA chain per output), any ks/stride/pad/Cin/Cout.
 * w: fp32 [ks][ks][Cin][Cout].  Used for Cin==1 heads, Cout==1 tail and strided convs. */
int mud_conv2d_direct(const mud_conv_args* a, void* stream);

/* Implicit-GEMM convolution on the matrix cores, ks in {1,3}, stride 1, pad ks/2.
 * fp32 operands are split on the fly into fp16 hi+lo (saturating at +-65504) and multiplied as hi*hi + hi*lo + lo*hi with
 * fp32 accumulation (v_mfma_f32_32x32x16_f16 x3): ~2^-22 relative error per product; a.prec selects the cheaper plan.
 * w: packed by mud_pack_weights().  Requires Cin % 4 == 0, ldx % 4 == 0, 16-byte aligned x.
 * For ks == 1 the (H, W) plane is treated as one flat axis of H*W positions (plain GEMM). */
int64_t mud_packed_weight_bytes(int ks, int Cin, int Cout);
/* src element (tap, ci, co) = src[tap*s_tap + ci*s_ci + co*s_co] (+ b*src_bstride elements).
 *   OIHW conv weight:  s_tap=1, s_ci=ks*ks, s_co=Cin*ks*ks;   NIN W[in,out]: s_ci=Cout, s_co=1;
 *   K^T of attention: rows of K as "co": s_ci=1, s_co=ldk;   V: s_ci=ldv, s_co=1.               */
int mud_pack_weights(const float* src, int64_t s_tap, int64_t s_ci, int64_t s_co, int64_t src_bstride,
                     int ks, int Cin, int Cout, int nbatch, void* dst, void* stream);
/* The same for a given arithmetic plan: MUD_PREC_FP8X (ks == 3 only) writes fp16 hi planes and the two e4m3 images
 * (w * 2^w_exp, (w - fp16(w)) * 2^(w_exp + 11)) in place of the lo planes; same size. */
int mud_pack_weights_prec(const float* src, int64_t s_tap, int64_t s_ci, int64_t s_co, int64_t src_bstride,
                          int ks, int Cin, int Cout, int nbatch, int prec, int w_exp, void* dst, void* stream);
/* Bytes of one packed operand for plan `prec`: MUD_PREC_16X3 / MUD_PREC_FP8X = mud_packed_weight_bytes; MUD_PREC_16X1 (ks == 3 only,
 * fp16 hi planes alone: mud_pack_weights_prec writes them) ceil(Cout/64) * ceil(Cin/16) * 9 * 2048 + 4096, half the steps' bytes.
 * -1 for a plan / ks pair that has no packed form. */
int64_t mud_packed_weight_bytes_prec(int ks, int Cin, int Cout, int prec);
int mud_conv2d_mfma(const mud_conv_args* a, void* stream);
/* 1 when mud_conv2d_mfma has plan `prec` for this launch (sizes, prologue mode, skip_w, sub2 are looked at), else 0. */
int mud_conv2d_mfma_prec_supported(const mud_conv_args* a, int prec);
/* Bytes of split-K workspace mud_conv2d_mfma would use for this call (0: the launch is not split). */
int64_t mud_conv2d_mfma_splitk_bytes(const mud_conv_args* a);
/* 1 when mud_conv2d_mfma takes res_up2 for this launch (ks, sub2, skip_w, sizes and the split-K policy are looked at), else 0. */
int mud_conv2d_mfma_res_up2_supported(const mud_conv_args* a);
/* 1 when mud_conv2d_mfma takes in_up2 for this launch (ks, sub2, skip_w, res_up2, pro_mode, the output size H x W, the tile that  */
/* size takes, a.prec and the split-K policy are looked at), else 0. */
int mud_conv2d_mfma_in_up2_supported(const mud_conv_args* a);
/* 1 when mud_conv2d_mfma takes in_s2d for this launch (ks, pro_mode, sub2, skip_w, res_up2, in_up2, Cin, the tile the view's size  */
/* takes, a.prec and the split-K policy are looked at), else 0. */
int mud_conv2d_mfma_in_s2d_supported(const mud_conv_args* a);
/* The workgroup tile mud_conv2d_mfma launches for a ks == 3 argument block (rows x 32 px x output channels, waves): it follows from  */
/* the workgroup count alone (B, H, W, Cout; Cin <= 64 for the one-row tile), never from the layer.  skip_w set: the fused skip conv  */
/* is built for 8X2, 16X1 and MT1 only, so its small grids take MT1.  in_up2 / in_s2d: H, W, Cin as the launch takes them; -1 where   */
/* the form is not built for the tile and a.prec.  -1 for ks != 3 or sizes <= 0.  Sizes, skip_w, in_up2, in_s2d and prec are looked   */
/* at, no pointer is dereferenced.  (The A/B knobs MUD_CONV_NO16 / MUD_CONV_NO8X1R are honoured; MUD_CONV_MT, which forces a tile on   */
/* plain launches, is not.)                                                                                                            */
#define MUD_TILE_8X2 0         /*  8 rows x 128 channels, 8 waves                     (an even number of 64-channel tiles) */
#define MUD_TILE_16X1 1        /* 16 rows x  64 channels, 8 waves                                                         */
#define MUD_TILE_MT2 2         /*  8 rows x  64 channels, 4 waves                                                         */
#define MUD_TILE_MT1 3         /*  4 rows x  64 channels, 4 waves                     (every grid too small for the others) */
#define MUD_TILE_8X1R 4        /*  8 rows x  64 channels, 8 waves of one row each     (Cout <= 64 and Cin <= 64)           */
int mud_conv2d_mfma_tile(const mud_conv_args* a);

/* ---- e4m3 range census of a convolution input (the precision guard of MUD_PREC_FP8X: mudiff_hip.precision).
 * MUD_PREC_FP8X converts every prologued activation a (and its fp16 remainder a - fp16(a)) to e4m3 at CONSTANT power-of-two
 * pre-scales; the cross terms are only right while |a| stays inside about [5e-4, 112].  This call mirrors the staging of
 * mud_conv2d_mfma (conv_mfma.hip, cm_stage4: fmaf(x, scale, shift), then the same fast SiLU, fp16 pieces saturating at +-65504)
 * on every element of the view and ACCUMULATES into `out` (a device struct; zero it once, every launch adds to it):
 *   n            elements seen
 *   n_over       |a|*2^CM_X_SA > 448  or  |a - fp16(a)|*2^CM_X_SAL > 448       (an e4m3 image saturates)
 *   n_under      0 < |a|*2^CM_X_SA < 2^-9                                      (below e4m3's smallest subnormal: flushes)
 *   n_fp16_over  |a| > 65504                                                   (the fp16 hi piece saturates, both plans)
 *   amax_bits    bit pattern of max |a| (fp32, zero-extended; merged with an integer max)
 * Integer counts merged with one atomic per counter per workgroup: the result does not depend on the order of arrival.
 * x: 16-byte aligned, C % 4 == 0, ldx % 4 == 0, ldx >= C, B*H*W*C/4 < 2^31.  pro_mode: MUD_PRO_NONE, MUD_PRO_AFFINE or
 * MUD_PRO_AFFINE_SILU; with an affine mode pro_scale / pro_shift are [B, pro_ld] rows (16-byte aligned, pro_ld % 4 == 0, >= C). */
typedef struct mud_census_args {
  const float* x; int B, H, W, C, ldx;
  const float* pro_scale; const float* pro_shift; int pro_ld; int pro_mode;
} mud_census_args;
typedef struct mud_census_out {
  uint64_t n, n_over, n_under, n_fp16_over, amax_bits;
} mud_census_out;
int mud_e4m3_census(const mud_census_args* a, mud_census_out* out, void* stream);

/* ---- FIR resampling (utils/op/upfirdn2d.cpp:20-31 + upfirdn2d_kernel.cu:109-209; python front
 *      ends backbones/up_or_down_sampling.py:149-262).
 * Plane form = the reference's pybind op: input [planes, H, W] (its [major, in_h, in_w, minor=1]),
 * kernel fp32 [kh, kw] on the device, same argument meaning as upfirdn2d(...). */
int mud_upfirdn2d(const float* in, int64_t planes, int H, int W, const float* kernel, int kh, int kw,
                  int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                  float* out, void* stream);
/* NHWC form used inside the generators: same filter maths on a view, optionally producing in ONE
 * pass both FIR(prologue(x)) (out_h) and FIR(x) (out_x) as ResnetBlockBigGANpp_Adagn needs
 * (layerspp.py:293-308).  kernel: host pointer to kh*kw floats (<= 64). Either output may be NULL. */
int mud_fir_nhwc(const float* x, int B, int H, int W, int C, int ldx, const float* kernel_host, int kh, int kw,
                 int up, int down, int pad0, int pad1,
                 const float* pro_scale, const float* pro_shift, int pro_ld, int pro_mode,
                 float* out_h, int ldh, float* out_x, int ldxo, void* stream);

/* ---- minibatch standard deviation of the critic (backbones/discriminator.py:246-254, stddev_feat = 1):
 * x view [B, hw, C]; samples b = g*M + m (g < group, M = B/group); out[b] = mean_{c,p} sqrt(var_g(x[g*M+m,p,c]) + 1e-8) */
int mud_minibatch_stddev(const float* x, int B, int64_t hw, int C, int ld, int group, float* out, void* stream);

/* ---- fused attention (layerspp.py:118-122): out[b,i,:] = sum_j softmax_j(q_i.k_j * scale) v_j, single head.
 * qkv: [B, N, ld] with q at +0, k at +C, v at +2C (the fused NIN_0|1|2 output); out [B, N, ldo].
 * Flash-style (no N x N matrix in memory), split-fp16 MFMA.  Head dims: see mud_attention_supported().
 * When batch x ceil(N/128) workgroups would leave most CUs idle (single-slice latency case) the keys are split over
 * up to 16 workgroups per query block and merged by a second tiny kernel; that needs `ws` (mud_attention_ws_bytes(),
 * 16-byte aligned).  ws == NULL always runs unsplit. */
int mud_attention_supported(int C);
int64_t mud_attention_ws_bytes(int B, int N, int C);   /* 0 = no workspace needed for this problem */
int mud_attention(const float* qkv, int B, int N, int C, int ld, float scale, float* out, int ldo, void* ws, void* stream);

/* ---- unfused attention pieces (used when the head dim is not supported above) and the G2 feature fusion (…feat.py:769-788) */
int mud_softmax_rows(float* s, int64_t rows, int n, int ld, void* stream);          /* in place */
int mud_mul(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int64_t npix, int C, void* stream);
/* out = g*att + (1-g)*other; views are [B, hw, C]; optional per-channel stats of `out` as in mud_conv_args */
int mud_gate_mix(const float* g, int ldg, const float* att, int lda, const float* other, int ldb,
                 float* out, int ldo, int B, int64_t hw, int C, double* stats, int stats_ld, void* stream);

/* ---- rows f1 / f3: bilinear resize of planes [P,H,W] -> [P,Ho,Wo] with torch F.interpolate(mode='bilinear',
 *      align_corners=False) semantics (engine/test_volume.py:274 slice -> image_size; engine/train.py:959 uncertainty map),
 *      and out = clamp(x*scale + shift, lo, hi) (the [-1,1] -> [0,1] mapping, engine/test_volume.py:281). */
/* row f4: Gaussian Fourier features of log(t) (layerspp.py:68-77, ncsnpp_generator_adagn_feat.py:288-289):
 * out[b, k] = sin(2*pi*W[k]*log(t[b])), out[b, n+k] = cos(...); out is [B, 2n]. */
int mud_fourier_embedding(const float* t, const float* W, float* out, int B, int n, void* stream);
int mud_resize_bilinear(const float* in, int64_t planes, int H, int W, int Ho, int Wo, float* out, void* stream);
int mud_affine_clamp(const float* x, int64_t n, float scale, float shift, float lo, float hi, float* out, void* stream);

/* ---- on-device evaluation metrics (mudiff_hip.metrics; the driver's --device_metrics).  They replace the host end of an
 *      evaluation: the global intensity range and 8-bit quantisation of engine/test.py:371-387 and the PSNR / SSIM / MAE of
 *      tools/metric_calc.py:28-53 (skimage defaults: 7x7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, data_range 1).
 *
 * out[0] = min, out[1] = max over a[0..na) and b[0..nb) (fp32), in one launch sequence; NaN in both if any input is NaN (np.min);
 * +inf / -inf for empty inputs.  ws: mud_value_range_ws_bytes() bytes, 4-byte aligned. */
int64_t mud_value_range_ws_bytes(void);
int mud_value_range(const float* a, int64_t na, const float* b, int64_t nb, float* out, void* ws, void* stream);
/* out[i] = (uint8) clip((x[i] - lo) / range * 255.0f, 0, 255), every step IEEE fp32 rounded once, truncation toward zero: bit-identical
 * to numpy's clip((s - gmin) / (gmax - gmin) * 255.0, 0, 255).astype(uint8) on fp32 s (engine/test.py:386-387) when the caller
 * passes lo = (float)gmin and range = (float)(gmax - gmin) with the difference taken in double.  range must be finite and > 0. */
int mud_quantize_u8(const float* x, int64_t n, float lo, float range, uint8_t* out, void* stream);
/* Per-slice sums of uint8 images pred, gt [n, H, W] (H, W >= 7):  sse[i] = sum (g-p)^2,  sae[i] = sum |g-p| (exact, int64), and
 * ssim_sum[i] = the fp64 sum of the per-pixel SSIM of (g/255, p/255) over the (H-6) x (W-6) interior (tools/metric_calc.py:44-48;
 * PSNR = 10 log10(255^2 H W / sse), SSIM = ssim_sum / ((H-6)(W-6)), MAE = sae / (255 H W)).  Window sums are exact integers;
 * the per-slice sum has a fixed order, so results are bit-identical run to run and independent of n.
 * ws: mud_slice_metrics_ws_bytes(n, H, W) bytes (-1 for bad sizes), 8-byte aligned. */
int64_t mud_slice_metrics_ws_bytes(int n, int H, int W);
int mud_slice_metrics_u8(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, int64_t* sse, int64_t* sae, double* ssim_sum,
                         void* ws, int64_t ws_bytes, void* stream);

/* ---- whole-volume scoring (mudiff_hip.volume_metrics; the volume pipeline's --gt_volume).  It extends the definitions of
 *      tools/metric_calc.py:40-47 (PSNR, SSIM with skimage defaults, MAE) to fp32 volumes in [0, 1]: a 7x7x7 uniform window, sample
 *      covariance (343/342), K1 = 0.01, K2 = 0.03, data_range 1, masked means over regions.
 *
 * pred, gt (fp32), region (uint8) and the optional std (fp32, may be NULL) are [Z, X, Y] with planes contiguous, Z, X, Y >= 7.  Voxel v
 * belongs to region k (0 <= k < nreg <= MUD_VM_MAX_REGIONS) when bit k of region[v] is set.  sums[(z * nreg + k) * MUD_VM_NQ + q] are
 * fp64 sums over the voxels of plane z in region k, with d = pred - gt and e = |d| taken in fp64:
 *   MUD_VM_N       the voxel count             MUD_VM_SSE  sum d^2        MUD_VM_SAE      sum e
 *   MUD_VM_N_INT   the interior voxel count    MUD_VM_SSIM sum of SSIM over the interior voxels (whole window inside the volume)
 *   MUD_VM_SS      sum std                     MUD_VM_SS2  sum std^2      MUD_VM_SSE_STD  sum std * e      (zero without std)
 * Window sums are fp64 in a fixed order per voxel and the per-plane sums have a fixed order: bit-identical run to run; the SSIM
 * expression is not contracted, so pred == gt gives SSIM exactly 1.  ws: mud_volume_metrics_ws_bytes(Z, X, Y, nreg) bytes (-1 for bad
 * sizes), 8-byte aligned. */
#define MUD_VM_MAX_REGIONS 8
#define MUD_VM_NQ 8
#define MUD_VM_N 0
#define MUD_VM_SSE 1
#define MUD_VM_SAE 2
#define MUD_VM_N_INT 3
#define MUD_VM_SSIM 4
#define MUD_VM_SS 5
#define MUD_VM_SS2 6
#define MUD_VM_SSE_STD 7
int64_t mud_volume_metrics_ws_bytes(int Z, int X, int Y, int nreg);
int mud_volume_metrics(const float* pred, const float* gt, const uint8_t* region, const float* std, int Z, int X, int Y, int nreg,
                       double* sums, void* ws, int64_t ws_bytes, void* stream);

/* ---- LPIPS, AlexNet backbone (lpips v0.1, net='alex', eval; tools/metric_calc.py:50-51) of uint8 grayscale pairs (mudiff_hip.lpips_net).
 * Weights are packed once into the kernels' layout: mud_lpips_packed_bytes() bytes, 16-byte aligned, written by mud_lpips_pack from
 * device fp32 tensors in torch layout: table[768] = the scaled input of level v in channel c at [c*256 + v] (fp32, built on the host),
 * conv_w[l] [Cout][Cin][k][k] and conv_b[l] [Cout] of torchvision AlexNet features.{0,3,6,8,10}, lin_w[l] [C] of lin{l}.model.1.
 * mud_lpips_u8: out[i*5 + l] = d_l of pair (pred[i], gt[i]) [n, H, W], H, W >= 31, in fp64; LPIPS = sum over l.  Convolutions in exact
 * fp32 (fp32-input MFMA), the head in fp64; fixed-order sums, so results are bit-identical run to run and independent of n.
 * ws: mud_lpips_ws_bytes(n, H, W) bytes (-1 for bad sizes), 16-byte aligned; out 8-byte aligned. */
int64_t mud_lpips_packed_bytes(void);
int mud_lpips_pack(const float* table, void* const* conv_w, void* const* conv_b, void* const* lin_w, void* packed, void* stream);
int64_t mud_lpips_ws_bytes(int n, int H, int W);
int mud_lpips_u8(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const void* packed, double* out, void* ws,
                 int64_t ws_bytes, void* stream);

/* ---- N-sample ensemble inference (mudiff_hip.ensemble; the drivers' --num_samples).  Every Gaussian of an ensemble is a pure function
 *      of (seed, slice, sample, step, kind, element), so results do not depend on batch size, chunking or rank count.
 * mud_randn_keyed: out[r*row_len + e] for row r with keys[2r..2r+1] = (slice s >= 0, sample j in [0, 2^31)) (device int64 [rows][2]):
 * Philox4x64-10 (numpy.random.Philox's algorithm and word order) with key (seed, 0x4D55444946460001) and counter
 * (e/4, s, (j << 32) | (step << 8) | kind, 0); lane l = e % 4 takes the word pair (w[2(l/2)], w[2(l/2)+1]) = (wa, wb),
 * u1 = ((wa >> 11) + 1) 2^-53, u2 = (wb >> 11) 2^-53, r = sqrt(-2 log u1), theta = 2 pi u2: r cos theta (even l), r sin theta (odd l),
 * in fp64, rounded once to fp32.  kind: 0 x_init, 1 z, 2 posterior noise, or 5 / 6 / 7 / 8 / 9 / 10: the draws of mud_kspace_constrain /
 * mud_slab_constrain / mud_slab_kspace_constrain / mud_band_constrain / mud_lowres_constrain / mud_sense_constrain, so that a caller can
 * inject what those entries draw, or 11: the measurement noise of mudiff_hip.sense (3 and 4, mud_known_constrain's, stay refused); step in
 * [0, 2^24); row_len > 0.
 * mud_ensemble_stats: samples [n][N][hw] -> mean, std [n][hw] (N >= 2, hw > 0): y = clamp(x*scale + shift, lo, hi) in fp32 (each step
 * rounded once, NaN kept), m = (sum_j y_j) / N and v = sum_j (y_j - m)^2 / (N - 1) in fp64 in sample order j = 0..N-1,
 * mean = (float)m, std = (float)sqrt(v); a NaN sample gives NaN in both.  No atomics: a fixed function of the samples. */
int mud_randn_keyed(float* out, int rows, int64_t row_len, const int64_t* keys, uint64_t seed, int step, int kind, void* stream);
int mud_ensemble_stats(const float* samples, int n, int N, int64_t hw, float scale, float shift, float lo, float hi, float* mean,
                       float* std, void* stream);

/* ---- per-pixel order statistics of an ensemble (mudiff_hip.ensemble.sample_ensemble(quantiles=); the volume pipeline's
 *      --ensemble_quantiles, --ensemble_center median and --coverage).
 * mud_ensemble_quantiles: samples [n][N][hw] -> out [K][n][hw] (2 <= N <= MUD_ENSEMBLE_QUANTILES_MAX_N, 1 <= K <=
 * MUD_ENSEMBLE_MAX_QUANTILES, hw > 0).  With y_(0) <= ... <= y_(N-1) a pixel's samples after mud_ensemble_stats' pre-map
 * y = clamp(x*scale + shift, lo, hi) in ascending order and q[k] in [0, 1]:
 *   h = (N - 1) * q[k],  i = min(floor(h), N - 2),  g = h - i,  out = (float)(y_(i) + g * (y_(i+1) - y_(i)))
 * in fp64 from h on, each operation rounded once (no contraction): q = 0.5 is the median for odd and even N, q = 0 the minimum.  A pixel
 * with a NaN sample gives NaN for every q; the sign of a zero is not specified.  q: HOST array of K finite fractions, read at call time
 * and passed as a kernel argument (no device allocation).  A sorting network in registers, no LDS, no atomics: a fixed function of the
 * samples. */
#define MUD_ENSEMBLE_MAX_QUANTILES 8
#define MUD_ENSEMBLE_QUANTILES_MAX_N 64
int mud_ensemble_quantiles(const float* samples, int n, int N, int64_t hw, float scale, float shift, float lo, float hi, const double* q,
                           int K, float* out, void* stream);

/* ---- interval coverage against a ground truth (mudiff_hip.volume_coverage; the volume pipeline's --coverage).
 * lo, hi, gt (fp32) and the optional region (uint8, bit k = region k as for mud_volume_metrics; may be NULL: every voxel is in every
 * region) are [Z, X, Y] with planes contiguous, X*Y*Z < 2^31; 1 <= nreg <= MUD_VM_MAX_REGIONS.  For the planes z0 <= z <= z1
 * (0 <= z0 <= z1 < Z; planes outside are never read) and the voxels v of plane z in region k,
 *   counts[((z - z0) * nreg + k) * MUD_VC_NC + c]:  MUD_VC_N        voxels where none of lo, hi, gt is a NaN (the five below are over these)
 *                                                   MUD_VC_BELOW    gt < lo            MUD_VC_ABOVE  gt > hi
 *                                                   MUD_VC_INSIDE   neither            MUD_VC_NONFINITE  voxels where one of the three is a NaN
 *   sums[((z - z0) * nreg + k) * MUD_VC_NS + s]:    MUD_VC_WIDTH    sum of (double)hi - (double)lo     MUD_VC_WIDTH_INSIDE  the same over `inside`
 * A voxel with a NaN is counted in MUD_VC_NONFINITE and in nothing else.  Partials per (plane, workgroup) are added in a fixed order, no
 * atomics: bit-identical run to run.  ws: (z1 - z0 + 1) * MUD_VC_PARTS * nreg * (MUD_VC_NC + MUD_VC_NS) * 8 bytes, 8-byte aligned. */
#define MUD_VC_NC 5
#define MUD_VC_NS 2
#define MUD_VC_PARTS 16
#define MUD_VC_N 0
#define MUD_VC_BELOW 1
#define MUD_VC_ABOVE 2
#define MUD_VC_INSIDE 3
#define MUD_VC_NONFINITE 4
#define MUD_VC_WIDTH 0
#define MUD_VC_WIDTH_INSIDE 1
int mud_volume_interval_coverage(const float* lo, const float* hi, const float* gt, const uint8_t* region, int Z, int X, int Y, int nreg,
                                 int z0, int z1, int64_t* counts, double* sums, void* ws, int64_t ws_bytes, void* stream);

/* ---- slice-coupled sampling noise (mudiff_hip.slice_coupling; the volume pipeline's --slice_coupling).
 * mud_randn_keyed_coupled: the keyed draws of neighbouring slices filtered along z.  With eta(s)[e] the fp32 value mud_randn_keyed gives
 * element e of a row keyed (slice s, sample m) under the same seed, step and kind,
 *   out[r*row_len + e] = (float) sum_{j=-R..R} w_|j| * eta(s_r + j)[e],
 * the products and the sum in fp64 in tap order j = -R..R, each rounded once (no contraction).  s_r + j wraps modulo 2^64 as the Philox
 * counter word, so the noise is stationary at a volume's first slices; the keys themselves obey mud_randn_keyed's rules.
 * half_taps: HOST array of radius + 1 finite fp64 weights w_0..w_R, read at call time and passed as a kernel argument (no device
 * allocation); radius in [0, MUD_COUPLING_MAX_RADIUS].  With sum_j w_|j|^2 = 1 (the caller's business: mudiff_hip.slice_coupling.
 * coupling_taps) every element stays N(0, 1) and rows d slices apart correlate by sum_j w_|j| w_|j+d|.  radius 0 with w_0 = 1 gives
 * mud_randn_keyed's bits. */
#define MUD_COUPLING_MAX_RADIUS 32
int mud_randn_keyed_coupled(float* out, int rows, int64_t row_len, const int64_t* keys, uint64_t seed, int step, int kind,
                            const double* half_taps, int radius, void* stream);

/* ---- sampling with a partly acquired target (mudiff_hip.known_region; GraphSampler.sample_keyed(known=)).
 * mud_known_constrain: re-imposes the known voxels on a reverse step's result at that step's noise level (RePaint, Lugmayr et al. 2022).
 * Rows are the slices of a batch, row_len contiguous fp32 values each.  With c = clamp(t[r] + toff, 0, ntab - 1) (mud_q_sample's rule),
 *   out[r][e] = mask[r][e] ? (clean ? known[r][e] : a_tab[c] * known[r][e] + s_tab[c] * eta[r][e]) : x_new[r][e],
 * the two products and the sum in fp32, each rounded once, in mud_q_sample's order: with the same eta the known part has mud_q_sample's
 * bits.  It is a select: whatever `known` holds where the mask is 0 (a NaN, an inf) never reaches out.  eta is `noise` [rows][row_len] when
 * that is given, else the value mud_randn_keyed gives element e of a row keyed keys[2r..2r+1] under (seed, step, kind): the same
 * counter, key and Box-Muller, drawn in the kernel, and only by the threads (4 consecutive elements each) that have a known element.
 * kind in [0, 15] (mud_randn_keyed itself accepts 0..2: 3 and 4 are this entry's, mudiff_hip.ops.KIND_KNOWN / KIND_RENOISE); step in
 * [0, 2^24).  mask: uint8 [rows][row_len], non-zero = known; NULL = known everywhere, x_new may then be NULL as well and the call is a
 * keyed q_sample of `known`.  out may be x_new or known.  With clean != 0 nothing is drawn: t, the tables, noise and keys may be NULL.
 * 16-byte loads and stores when row_len % 4 == 0 and every pointer is 16-byte (the mask: 4-byte) aligned, else element by element.
 * MUD_ERR_ARG before any launch for rows <= 0, row_len <= 0, ntab <= 0, a kind or step out of range, a null pointer that is needed, and
 * neither noise nor keys.
 * mud_known_coverage: out (uint8 [Z][Y][X]) = 1 where the destination voxel (i, j, k) of a resampling by the matrix m of
 * mud_volume_regrid (12 doubles on the host, finite) has a source coordinate p with 0 <= p_a <= S_a - 1 on all three axes, else 0;
 * p in fp64 as mud_volume_regrid_cubic forms it.  There the trilinear and the cubic footprint need no zero padding: the voxel was
 * interpolated from acquired voxels alone.  Both sizes positive, X*Y*Z < 2^31. */
int mud_known_constrain(const float* x_new, const float* known, const uint8_t* mask, const float* noise, const int64_t* keys, uint64_t seed,
                        int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab, int clean,
                        float* out, int rows, int64_t row_len, void* stream);
int mud_known_coverage(const double* m, int SX, int SY, int SZ, int X, int Y, int Z, uint8_t* out, void* stream);

/* ---- sampling a target acquired undersampled in k-space (mudiff_hip.kspace; GraphSampler.sample_keyed(kspace=)).
 * F is the unitary 2D DFT of an S x S slice: F(x)[u][v] = (1/S) sum_{j,k} x[j][k] exp(-2 pi i (u j + v k) / S), DC at [0][0], S a power of
 * two in [16, 512]; the scale 1/S is an exact power of two.  Complex data is interleaved (re, im) fp32, the layout of torch.complex64.
 * Radix-4 passes (and one radix-2 layer when log2 S is odd) in LDS with twiddles correctly rounded from fp64; every product and sum is
 * rounded once (no contraction); no atomics; a slice's result depends on that slice's operands alone, not on the batch around it.
 * mud_fft2_c2c: out[r] = F(in[r]) (inverse != 0: F^H) for rows slices [rows][S][S]; in place (out == in) is allowed.  Two launches.
 * mud_fft2_r2c: the same with `in` real fp32 [rows][S][S]: the bits of mud_fft2_c2c on (in, 0).  Not in place.
 * mud_kspace_constrain: the data-consistency step for measurements y = mask .* F(k).  With c = clamp(t[r] + toff, 0, ntab - 1),
 *   out[r] = x_new[r] - Re F^H[ mask ? F(x_new[r] - s_tab[c] * eta[r]) - a_tab[c] * y[r] : 0 ]
 * and with clean != 0  out[r] = x_new[r] - Re F^H[ mask ? F(x_new[r]) - y[r] : 0 ]  (nothing drawn: t, the tables, noise and keys may be
 * NULL).  Where the mask is 0 the residual is an exact 0, and a correction that is 0 leaves x_new's bits: an all-zero mask returns x_new
 * bit for bit.  y: complex [rows][S][S]; mask: uint8 [mask_rows][S][S], non-zero = measured, mask_rows 1 (shared) or rows; work: a
 * complex workspace [rows][S][S] of the caller's, overwritten.  eta is `noise` [rows][S][S] when given, else the value mud_randn_keyed
 * gives element e of a row of S * S elements keyed keys[2r..2r+1] under (seed, step, kind) - counter words (e / 4, slice, sample << 32 |
 * step << 8 | kind, 0), drawn in the kernel by the thread that loads elements 4b..4b+3; kind in [0, 15] (mudiff_hip.ops.KIND_KSPACE =
 * 5 is this entry's), step in [0, 2^24).  out may be x_new.  Three launches: rows forward (d = x_new - s * eta fused into the load),
 * columns forward -> residual -> columns inverse inside LDS, rows inverse (out = x_new - Re(.) fused into the store).
 * MUD_ERR_ARG before any launch for an S that is not a power of two in [16, 512], rows <= 0 or rows * S * S >= 2^31, mask_rows outside
 * {1, rows}, ntab <= 0, a kind or step out of range, a null pointer that is needed, neither noise nor keys, x_new / out / noise not
 * 16-byte aligned, and a work that is one of the other operands. */
int mud_fft2_c2c(const float* in, float* out, int rows, int S, int inverse, void* stream);
int mud_fft2_r2c(const float* in, float* out, int rows, int S, int inverse, void* stream);
int mud_kspace_constrain(const float* x_new, const float* y, const uint8_t* mask, int mask_rows, const float* noise, const int64_t* keys,
                         uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab,
                         int clean, float* out, float* work, int rows, int S, void* stream);

/* ---- sampling a target acquired with thick slices (mudiff_hip.thick; GraphSampler.sample_keyed(thick=)).
 * A group (a slab) names up to L rows of the batch, its thin slices, with weights w_l > 0 (the slice profile) and gains
 * g_l = w_l / sum_m w_m^2, formed by the caller in fp64 and rounded once; its measurement y[g] is sum_l w_l k_l per element.  The host
 * tables, read at call time (they travel as kernel arguments): members int32 [groups][L], a row index or -1 = unused; weights and gains
 * fp32 [groups][L].  No row is in two groups or twice in one, so the groups' rows are orthogonal and the step is an exact projection.
 * mud_slab_constrain: with c = clamp(t[first member of g] + toff, 0, ntab - 1), for every group g and element e
 *   r = sum_l w_l (x_new[m_l][e] - s_tab[c] * eta[m_l][e]) - a_tab[c] * y[g][e]      (clean != 0:  r = sum_l w_l x_new[m_l][e] - y[g][e])
 *   out[m_l][e] = x_new[m_l][e] - g_l * r                                            for every member l,
 * in fp32, every product and sum rounded once (no contraction), the sum over l from 0 in the table's order whatever the rows' positions:
 * a group's result depends on its own rows, table and keys alone, not on where its rows sit or on what else is in the batch.  A
 * correction g_l * r that compares equal to 0 leaves x_new's bits, and a row of no group is copied bit for bit (nothing when out is
 * x_new, which is allowed).  eta is `noise` [rows][row_len] when given, else the value mud_randn_keyed gives element e of a row keyed
 * keys[2r..2r+1] under (seed, step, kind), drawn by the thread that owns elements 4b..4b+3 of the group (Philox block b of each member
 * row); kind in [0, 15] (mudiff_hip.ops.KIND_THICK = 6 is this entry's), step in [0, 2^24).  With clean != 0 nothing is drawn: t, the
 * tables, noise and keys may be NULL.  One thread owns 4 consecutive elements of one group and walks its members twice (accumulate,
 * then store); 16-byte loads and stores when row_len % 4 == 0 and x_new, y, noise and out are 16-byte aligned, else element by element.
 * One launch per 32 groups or 128 members; no atomics, no LDS, no allocation on the device.
 * mud_slab_average: avg[g][e] = sum_l w_l x[m_l][e] under the same tables, order and rounding (avg: fp32 [groups][row_len]).
 * MUD_ERR_ARG before any launch or copy, naming the argument, for a member outside [0, rows) (other than -1), a row named twice, a group
 * with no member, a weight or gain that is not finite and positive, L outside [1, MUD_SLAB_MAX_MEMBERS], groups outside [0, rows]
 * (average: [1, rows]), rows * row_len >= 2^31, ntab <= 0, a kind or step out of range, a null pointer that is needed, and neither noise
 * nor keys. */
#define MUD_SLAB_MAX_MEMBERS 16
int mud_slab_constrain(const float* x_new, const float* y, const int32_t* members, const float* weights, const float* gains, int groups, int L,
                       const float* noise, const int64_t* keys, uint64_t seed, int step, int kind, const int64_t* t, int toff,
                       const float* a_tab, const float* s_tab, int ntab, int clean, float* out, int rows, int64_t row_len, void* stream);
int mud_slab_average(const float* x, const int32_t* members, const float* weights, int groups, int L, float* avg, int rows, int64_t row_len,
                     void* stream);

/* ---- sampling a target acquired as accelerated thick slices (mudiff_hip.multislice; GraphSampler.sample_keyed(constraint=
 *      SlabKSpaceRows)).  The composite of the two models above: a group (a slab) of up to L rows with weights w_l
 * and gains g_l = w_l / sum_m w_m^2 (the tables of mud_slab_constrain), whose average was measured in k-space on a mask:
 * y[g] = mask .* F(sum_l w_l k_l).  A A^H = (sum w^2) mask, so the step is still an exact projection.
 * mud_slab_kspace_constrain: with c = clamp(t[first member of g] + toff, 0, ntab - 1), for every group g
 *   d = sum_l w_l (x_new[m_l] - s_tab[c] * eta[m_l])                                  (clean != 0:  d = sum_l w_l x_new[m_l])
 *   C = Re F^H[ mask ? F(d) - a_tab[c] * y[g] : 0 ]                                   (clean != 0:  ... - y[g])
 *   out[m_l] = x_new[m_l] - g_l * C                                                   for every member l,
 * in fp32, every product and sum rounded once (no contraction), the sum over l from 0 in the table's order whatever the rows'
 * positions, the transforms those of mud_kspace_constrain: a group's result depends on its own rows, table and keys alone, and with
 * L = 1, w = g = 1 it has mud_kspace_constrain's bits.  A correction g_l * C that compares equal to 0 leaves x_new's bits (an all-zero
 * mask returns x_new bit for bit), and a row of no group is copied bit for bit (nothing when out is x_new, which is allowed).
 * y: complex [groups][S][S]; mask: uint8 [mask_rows][S][S], mask_rows 1 (shared) or groups; work: a complex workspace [groups][S][S]
 * of the caller's, overwritten.  eta is `noise` [rows][S][S] when given, else the value mud_randn_keyed gives element e of a row keyed
 * keys[2r..2r+1] under (seed, step, kind), drawn by the thread that loads elements 4b..4b+3 of that row; kind in [0, 15]
 * (mudiff_hip.ops.KIND_MULTISLICE = 7 is this entry's), step in [0, 2^24).  Three launches per 32 groups or 128 members: rows forward
 * (the members' sum fused into the load), mud_kspace_constrain's column pass by group, rows inverse (the members' correction fused
 * into the store).  No atomics, no allocation on the device.
 * MUD_ERR_ARG before any launch or copy for every refusal of mud_kspace_constrain (S, rows * S * S, alignment, work, kind, step, null
 * pointers, neither noise nor keys; mask_rows outside {1, groups}) and of mud_slab_constrain (members, weights, gains, L, groups). */
int mud_slab_kspace_constrain(const float* x_new, const float* y, const uint8_t* mask, int mask_rows, const int32_t* members,
                              const float* weights, const float* gains, int groups, int L, const float* noise, const int64_t* keys,
                              uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab,
                              int ntab, int clean, float* out, float* work, int rows, int S, void* stream);

/* ---- sampling a target given as a thick-slice volume of its own geometry (mudiff_hip.thick_volume; GraphSampler.sample_lockstep,
 *      DESIGN.md section 5.29).  Thick slice j of m is a weighted average of thin slices of a stack of n, y_j = sum_i A_ji k_i per
 * element; thick slices may cut thin slices in fractions and overlap, so G = A A^T is banded (bandwidth bw) and symmetric positive
 * definite.  The tables (struct mud_band_tables) are built by the caller in fp64, rounded once and kept in DEVICE memory: the CSR of A
 * by thick slice (start int32 [m + 1], member int32 [nnz] = thin index, w fp32 [nnz]), the CSR of A^T by thin slice (tstart int32
 * [n + 1], tmember int32 [nnz] = thick index ascending, tw fp32 [nnz]) and the banded Cholesky factor of G, lc fp32 [m][bw + 1] with
 * lc[j][0] = 1 / L[j][j] and lc[j][k] = L[j][j - k].  A set is one sample's whole stack: x, noise, out are [sets][n][row_len], keys
 * [sets * n][2], t [sets * n], y [m][row_len] (shared by the sets), work [sets][m][row_len] (the caller's, overwritten).
 * mud_band_constrain: with c = clamp(t[first row of the set] + toff, 0, ntab - 1), a = a_tab[c], s = s_tab[c] (clean != 0: a = 1, s = 0,
 * nothing drawn), per element of a set
 *   forward,  j = 0..m-1:  r_j = sum_s w_js (x[member_js] - s * eta[member_js]) - a * y_j,   v_j = (r_j - sum_{k=1..bw} lc[j][k] v_{j-k}) * lc[j][0]
 *   backward, j = m-1..0:  u_j = (v_j - sum_{k=1..bw} lc[j+k][k] u_{j+k}) * lc[j][0]
 *   scatter,  every i:     c = sum_j tw_ji u_j,   out_i = (c == 0 ? x_i : x_i - c)
 * in fp32, every product and sum rounded once (no contraction), every sum from 0 in the table's order (k ascending): the orthogonal
 * projection x - A^T G^-1 (A (x - s eta) - a y).  A thin slice under no thick slice is copied bit for bit (nothing when out is x, which
 * is allowed).  eta is `noise` when given, else the value mud_randn_keyed gives element e of the row keyed keys[2r..2r+1] under (seed,
 * step, kind), drawn by the thread that owns elements 4b..4b+3 of the set's column (Philox block b of each row); kind in [0, 15]
 * (mudiff_hip.ops.KIND_BAND = 8 is this entry's), step in [0, 2^24).  One thread owns 4 consecutive elements of one set's whole column;
 * grid (ceil(row_len / 4 / 256), sets); 16-byte accesses when row_len % 4 == 0 and x, y, noise, out, work are 16-byte aligned, else
 * element by element.  One launch; no atomics, no LDS, no allocation: a set's result depends on its own rows, keys and the tables alone.
 * mud_band_measure: ax[set][j] = sum_s w_js x[set][member_js] in the same order and rounding (ax: fp32 [sets][m][row_len]).
 * MUD_ERR_ARG before the launch for m outside [1, MUD_BAND_MAX_M], n outside [1, MUD_BAND_MAX_N], bw outside [0, min(MUD_BAND_MAX_BW,
 * m - 1)], nnz outside [m, m * MUD_BAND_MAX_MEMBERS], sets outside [1, 65535], sets * max(m, n) * row_len >= 2^31, ntab <= 0, a kind or
 * step out of range, a null pointer that is needed, neither noise nor keys, and a work or out that overlaps another operand (out == x
 * excepted).  The tables' contents cannot be read on the host: the kernel skips an index outside [0, n) or [0, m).
 * Replaces nothing in the reference (it has no measurement model); new with section 5.29. */
#define MUD_BAND_MAX_MEMBERS 32
#define MUD_BAND_MAX_BW 8
#define MUD_BAND_MAX_M 256
#define MUD_BAND_MAX_N 512
typedef struct mud_band_tables {
  int m, n, bw, nnz;
  const int32_t* start;
  const int32_t* member;
  const float* w;
  const int32_t* tstart;
  const int32_t* tmember;
  const float* tw;
  const float* lc;
} mud_band_tables;
/* mud_band_constrain: new (no counterpart in the reference) */
int mud_band_constrain(const float* x, const float* y, const mud_band_tables* tab, const float* noise, const int64_t* keys, uint64_t seed, int step,
                       int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab, int clean, float* out, float* work,
                       int sets, int64_t row_len, void* stream);
/* mud_band_measure: new (no counterpart in the reference) */
int mud_band_measure(const float* x, const mud_band_tables* tab, float* ax, int sets, int64_t row_len, void* stream);

/* ---- sampling a target given as a volume coarser than the stack in all three axes (mudiff_hip.lowres_volume; GraphSampler.
 *      sample_lockstep).  Coarse voxel (jz, jy, jx) is a separable weighted average of fine voxels,
 * y = (A_z (x) A_y (x) A_x) k, with one struct mud_band_tables per axis: tab_z over the n = tab_z.n thin slices of a set, tab_y over
 * the H image rows (tab_y.n == H), tab_x over the W image columns (tab_x.n == W).  A A^T = G_z (x) G_y (x) G_x, so the orthogonal
 * projection x - A^T (A A^T)^-1 (A (x - s eta) - a y) is one banded Cholesky solve per axis.  x, noise, out are [rows][H][W] with
 * rows = sets * n, sample-major as for mud_band_constrain (keys [rows][2], t [rows]); y is [m_z][m_y][m_x], shared by the sets; work
 * is the caller's, mud_lowres_ws_floats(sets, n, m_z, m_y, m_x) floats (P [rows][m_y][m_x], then U [sets][m_z][m_y][m_x]), overwritten.
 * mud_lowres_constrain, four launches, with a, s of the level of the set's first row as in mud_band_constrain (clean: a = 1, s = 0):
 *   1. P[r][jy][jx] = sum_sx wx (sum_sy wy (x - s * eta)[r][yy][xx]): per column the image rows of coarse row jy in tab_y's order, then
 *      the columns of jx in tab_x's order.  eta: `noise`, else mud_randn_keyed's value for element yy * W + xx of the row keyed
 *      keys[2r..2r+1] under (seed, step, kind) (mudiff_hip.ops.KIND_LOWRES = 9 is this entry's); drawn once per coarse row that covers it
 *   2. per set and coarse column: R_j = sum_s wz P[member] - a * y_j in tab_z's order, then mud_band_constrain's forward and backward
 *      pass with tab_z.lc
 *   3. per set and coarse slice: the same two passes with tab_y.lc along jy, then with tab_x.lc along jx -> U
 *   4. c = sum_jz twz (sum_jy twy (sum_jx twx U[jz][jy][jx])) with the transposed tables, each index ascending; out = (c == 0 ? x : x - c)
 * in fp32, every product and sum rounded once, every sum from 0.  out may be x; then an element under no coarse voxel (a thin slice, an
 * image row or a column outside every support) is not written.  16-byte accesses when W % 4 == 0 and x, noise, out are 16-byte aligned,
 * else element by element.  No atomics, no allocation: a set's result depends on its own rows, keys and the tables alone.
 * mud_lowres_measure: ax [sets][m_z][m_y][m_x] = A x by passes 1 and 2's sums alone (no eta, no y, no solve); work: rows * m_y * m_x floats.
 * mud_lowres_ws_floats: the floats of work; -1 for a size < 1.
 * MUD_ERR_ARG before any launch for a null pointer that is needed, per axis the limits of mud_band_constrain (m of an axis 0 among
 * them), tab_y.n != H, tab_x.n != W, tab_z.n not dividing rows, rows > 65535, rows * H * W >= 2^31, ntab <= 0, a kind or step out of
 * range, neither noise nor keys, and a work or out that overlaps another operand (out == x excepted).  The kernels skip a table index
 * outside its axis.  Replaces nothing in the reference (it has no measurement model); new with section 5.31. */
/* mud_lowres_constrain: new (no counterpart in the reference) */
int mud_lowres_constrain(const float* x, const float* y, const mud_band_tables* tab_z, const mud_band_tables* tab_y,
                         const mud_band_tables* tab_x, int H, int W, int rows, float* work, const float* noise, const int64_t* keys,
                         uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab,
                         int clean, float* out, void* stream);
/* mud_lowres_measure: new (no counterpart in the reference) */
int mud_lowres_measure(const float* x, const mud_band_tables* tab_z, const mud_band_tables* tab_y, const mud_band_tables* tab_x, int H,
                       int W, int rows, float* work, float* ax, void* stream);
/* mud_lowres_ws_floats: new (no counterpart in the reference) */
int64_t mud_lowres_ws_floats(int sets, int n, int m_z, int m_y, int m_x);

/* ---- sampling a target acquired accelerated on several coils (mudiff_hip.sense; GraphSampler.sample_keyed).
 * S a power of two in [16, 512], F the unitary 2D DFT of mud_fft2_c2c.  maps: complex64 [map_rows][coils][S][S], the coil sensitivities
 * C_c (map_rows 1: one set for every row, else rows); mask: uint8 [mask_rows][S][S], non-zero = measured, taken as it is (C_c x is
 * complex: pass the pattern, not its Hermitian symmetrisation).  A x = (mask .* F(C_c x))_c, A^H z = Re sum_c conj(C_c) F^H z_c and
 * N = A^H A.
 * mud_sense_measure: y [rows][coils][S][S] complex64 = A x for x fp32 [rows][S][S]: rows forward with the multiply by C_c fused into the
 *   load, then columns forward, the mask applied in the store.
 * mud_sense_adjoint: out fp32 [rows][S][S] = A^H y (no mask: y is what mud_sense_measure gave, zero where nothing was measured).  y is
 *   the transform's workspace and is OVERWRITTEN.  Columns inverse in place, then rows inverse with the coil sum in registers, coil 0 first.
 * mud_sense_constrain: with a, s = a_tab[c], s_tab[c] at c = clamp(t[r] + toff, 0, ntab - 1) (clean: a = 1, s = 0, no draw) and eta as
 *   for mud_kspace_constrain (mudiff_hip.ops.KIND_SENSE = 10 is this entry's kind),
 *       b = N (x_new - s eta) - a ahy,    (I + lambda N) e = b by exactly `iters` conjugate-gradient steps from e = 0,    out = x_new - lambda e:
 *   the minimiser of |x - x_new|^2 + lambda |A (x - s eta) - a y|^2 for ahy = A^H y (fp32 [rows][S][S]).  One application of N is three
 *   launches (rows forward: the vector's formation fused into the load; columns forward, mask, inverse in LDS; rows inverse: the coil sum
 *   in registers, q = p + lambda N p or b = N v - a ahy and the workgroup's partial of p.q or b.b fused into the store), one more per
 *   iteration for e += alpha p, r -= alpha q and the partial of r.r, p = r + beta p being fused into the next rows-forward load.  Every
 *   scalar is per row, summed in fp64 from the fp32 partials [row][tile] in tile order by each workgroup: no atomics, no host read, a
 *   fixed sequence of 4 + 4 iters launches; a row's result depends on its own operands alone.  A row whose b is exactly 0, whose r.r
 *   reaches exactly 0 or whose p.q is 0 is frozen from then on.  out = x_new's bits where lambda e compares equal to 0 (a zero mask,
 *   zero maps, lambda = 0; a -0 included); out may be x_new.  cg_res[rows] = |r_iters| / |b|, 0 for a frozen row.  work:
 *   mud_sense_ws_floats(rows, coils, S) floats of the caller's, overwritten (the spectra [rows][coils][S][S], r, p, q, e, the partials).
 * mud_sense_ws_floats: the floats of work; -1 for a size that is refused.
 * MUD_ERR_ARG before any launch for every refusal of mud_kspace_constrain, coils outside [1, MUD_SENSE_MAX_COILS], map_rows outside
 * {1, rows}, iters outside [1, 64], a lambda that is negative or not finite, rows * coils * S * S >= 2^31, a null pointer that is needed,
 * a misaligned operand (x_new, ahy, out, noise, work: 16 bytes; maps, y: 8) and a work that overlaps an operand.  Replaces nothing in
 * the reference (it has no measurement model); new with section 5.32. */
#define MUD_SENSE_MAX_COILS 32
/* mud_sense_constrain: new (no counterpart in the reference) */
int mud_sense_constrain(const float* x_new, const float* ahy, const uint8_t* mask, int mask_rows, const float* maps, int map_rows, int coils,
                        float lambda, int iters, const float* noise, const int64_t* keys, uint64_t seed, int step, int kind, const int64_t* t,
                        int toff, const float* a_tab, const float* s_tab, int ntab, int clean, float* out, float* cg_res, float* work, int rows,
                        int S, void* stream);
/* mud_sense_measure: new (no counterpart in the reference) */
int mud_sense_measure(const float* x, const float* maps, int map_rows, int coils, const uint8_t* mask, int mask_rows, float* y, int rows, int S,
                      void* stream);
/* mud_sense_adjoint: new (no counterpart in the reference) */
int mud_sense_adjoint(float* y, const float* maps, int map_rows, int coils, float* out, int rows, int S, void* stream);
/* mud_sense_ws_floats: new (no counterpart in the reference) */
int64_t mud_sense_ws_floats(int rows, int coils, int S);

/* ---- through-plane roughness of a volume (mudiff_hip.volume_through_plane; the volume pipeline's --through_plane).
 * vol (fp32) and the optional mask (uint8, may be NULL: every voxel is inside; else non-zero is inside) are [Z, X, Y] with planes
 * contiguous, X*Y*Z < 2^31.  For the planes z0 <= z <= z1 (0 <= z0 <= z1 < Z; planes outside are never read),
 * sums[(z - z0) * MUD_TP_NQ + q] are the counts and fp64 sums, over the voxels v of plane z that are inside, of
 *   MUD_TP_N_DZ / _S_DZ    |V[z+1] - V[z]|               where z < z1 and the voxel above is inside
 *   MUD_TP_N_DZZ / _S_DZZ  |(V[z+1] - 2 V[z]) + V[z-1]|  where z0 < z < z1 and the voxels above and below are inside
 *   MUD_TP_N_DX / _S_DX    |V[x+1] - V[x]|               where x + 1 < X and that neighbour is inside
 *   MUD_TP_N_DY / _S_DY    |V[y+1] - V[y]|               where y + 1 < Y and that neighbour is inside
 * with every difference taken in fp64 from the fp32 values.  Partials per (plane, workgroup) are added in a fixed order, no atomics:
 * bit-identical run to run.  ws: (z1 - z0 + 1) * MUD_TP_PARTS * MUD_TP_NQ * 8 bytes, 8-byte aligned. */
#define MUD_TP_NQ 8
#define MUD_TP_PARTS 16
#define MUD_TP_N_DZ 0
#define MUD_TP_S_DZ 1
#define MUD_TP_N_DZZ 2
#define MUD_TP_S_DZZ 3
#define MUD_TP_N_DX 4
#define MUD_TP_S_DX 5
#define MUD_TP_N_DY 6
#define MUD_TP_S_DY 7
int mud_volume_through_plane(const float* vol, const uint8_t* mask, int Z, int X, int Y, int z0, int z1, double* sums, void* ws,
                             int64_t ws_bytes, void* stream);

/* ---- on-device NIfTI intake and re-assembly of the volume pipeline (mudiff_hip.volume_intake; --device_intake, mudiff_hip.cohort).
 * A volume is passed exactly as the file stores it: X x Y x Z voxels, x fastest ([Z][Y][X] in C terms), 16-byte aligned, X*Y*Z < 2^31,
 * in the NIfTI datatype MUD_NIFTI_* (little-endian), with the header's scl_slope / scl_inter.  A voxel's value is
 * float32(double(raw) * slope + inter), product and sum rounded separately, when scaling applies (slope finite and not 0, and not
 * slope 1 with inter 0: volume.read_nifti's rule), else float32(raw).  Voxels with value != 0 are `selected` (a NaN is).
 *
 * mud_volume_census: the order statistics of the selected values, as one device record (8-byte aligned):
 *   n, n_nonfinite (selected NaN / inf), min and max (0 when n is 0), and for each fraction q[i] in [0, 1] (i < nq <= MUD_VI_MAX_RANKS; a
 *   host array) the exact sorted values at the ranks first_rank[i] .. first_rank[i] + count[i] - 1 = [r - 8, r + 7] clipped to [0, n),
 *   r = floor((n - 1) * q[i]) in fp64 on the device: window[i][0 .. count[i]).  A radix select (8-bit digits, four histogram passes
 *   over the volume and one gathering pass): exact for any tie structure, no host round trip, no sort of the volume.  NaN sorts last.
 *   ws: mud_volume_census_ws_bytes() bytes, 8-byte aligned.
 * mud_volume_slab_normalise: out[i][x][y] (fp32 [s1 - s0 + 1][X][Y]) = clip((v - lo) / den, 0, 1) * 2 - 1 of the voxel (x, y, s0 + i),
 *   every step in fp32 and rounded once, the division correctly rounded; NaN stays NaN.  den is hi - lo as the host forms it (fp32).
 *   With `degenerate` != 0 (no selected voxels, or a flat volume) the slab is zeros.  Needs 0 <= s0 <= s1 < Z.
 * mud_volume_slab_zscore: the same slab under the training normalisation (--norm zscore): out[i][x][y] = clamp((v - mean) / std, -3, 3) / 3,
 *   every step in fp32 and rounded once, both divisions correctly rounded (the last one is a division by 3, not a product with 1 / 3);
 *   NaN stays NaN.  mean / std: the fp32 moments of the selected voxels as the host forms them (volume_intake.zscore_moments; 0 / 1 for
 *   no selected voxels, std 1 for a flat volume); std must not be 0.  Needs 0 <= s0 <= s1 < Z.
 * mud_volume_assemble: planes [s1 - s0 + 1][X][Y] (fp32) -> vol [Z][Y][X] (file order): zeros, except the planes s0..s1.  planes2 / vol2:
 *   an optional second stack (an ensemble's std) assembled the same way; both NULL or both given.
 * mud_volume_regrid (--regrid): a volume src of SX x SY x SZ stored voxels that lies on another voxel grid -> out, fp32 [Z][Y][X] in file
 *   order on the reference grid (the first input's), ready for the entry points above as MUD_NIFTI_F4 with slope 1, inter 0.  It lifts
 *   the reference's check that all inputs share one shape (engine/test_volume.py:262-263) for volumes whose world coordinates agree; it
 *   does not register.  m: 12 doubles on the host, the row-major 3 x 4 matrix inv(source affine) * (reference affine) that takes a
 *   reference voxel index (i, j, k) to a source voxel coordinate p = m * (i, j, k, 1), evaluated in fp64.
 *   mode 0, trilinear: f = floor(p), w = p - f; out = float32 of the fp64 sum over the 8 neighbours f + {0, 1}^3 of value * weight (x
 *   fastest), the weight being the product of w or 1 - w per axis.  A neighbour outside the source counts as 0 (zero padding: continuous
 *   at the border); one whose weight is exactly 0 is not read, so identities and integer shifts are bit-exact, next to a NaN too.
 *   mode 1, nearest (label volumes): the value at floor(p + 0.5) per axis, 0 outside the source.
 *   Both sizes obey X*Y*Z < 2^31; m must be finite.
 * mud_volume_bspline_coeffs, mud_volume_regrid_cubic (--regrid_interp cubic; no reference counterpart): mode 0 of
 *   mud_volume_regrid with a cubic B-spline in place of the trilinear kernel, in two steps.
 *   _bspline_coeffs: coeffs (device fp64 [SZ][SY][SX], 16-byte aligned, not vol) = the cubic B-spline coefficients of the stored volume
 *     under mirror (whole-sample symmetric) boundaries.  s = double(the value of a stored voxel), 0 for a non-finite value; nonfinite
 *     (device uint32, cleared first) counts those.  Every line s[0 .. N-1], along x, then y, then z, is replaced as follows, with
 *     z = sqrt(3) - 2 formed once on the host and every product and sum rounded separately (no fused multiply-add): for N == 1, c = s;
 *     else g[i] = 6 * s[i]; a = sum over k = 0 .. 2N-3, in increasing k, of zk * g[m(k)], where zk starts at 1 and is multiplied by z
 *     after each term and m(k) = k for k <= N-1, else 2N-2-k; c+[0] = a / (1 - zk) with the final zk; c+[i] = g[i] + z * c+[i-1];
 *     c[N-1] = (z / (z * z - 1)) * (c+[N-1] + z * c+[N-2]); c[i] = z * (c[i+1] - c+[i]) for i = N-2 .. 0.  No axis has a maximum length
 *     (the x pass moves along its lines in chunks staged in LDS, the y and z passes run one thread per line).
 *   _regrid_cubic: out, fp32 [Z][Y][X], from coeffs and the stored volume src they were made from (same size, datatype, slope, inter).
 *     m: the matrix of mud_volume_regrid; p = m * (i, j, k, 1) in fp64, ((m0 * i + m1 * j) + m2 * k) + m3 per axis, every product and sum
 *     rounded separately.  out = +0 when some axis does not satisfy 0 <= p_a <= S_a - 1 (no extrapolation), and when every in-volume
 *     neighbour of non-zero weight among the 8 trilinear neighbours of p (mode 0 of mud_volume_regrid) is a voxel whose value is 0: the
 *     background guard, so that the ringing of the spline creates no non-zero voxel where trilinear resampling leaves exact zeros.
 *     Otherwise f = floor(p), t = p - f, the weights b0 .. b3 of mud_volume_bias_* at t apply to the coefficient indices f-1 .. f+2 per
 *     axis, mirrored at each end (i < 0 -> -i, i > S-1 -> 2 (S-1) - i, and once more -i should that be negative; every index is 0 for
 *     S == 1), and out = float32(clamp(sum, lo, hi)), the fp64 sum running over the 4 x 4 x 4 support, z outermost and x fastest, of
 *     ((bx * by) * bz) * c.  lo, hi: finite, lo <= 0 <= hi; the caller passes the range of the source's finite values widened to contain
 *     0 (mud_volume_fg_range yields it), which keeps the overshoot of the spline at an edge inside the values the volume has.
 *   Both sizes obey X*Y*Z < 2^31; m must be finite.  No atomics on floating-point values: the same bits on every run.
 * mud_volume_joint_hist (--coregister): the joint histogram a rigid registration search evaluates, between a
 *   fixed volume (X x Y x Z stored voxels) and a moving one (SX x SY x SZ) seen through m, the matrix of mud_volume_regrid (fixed voxel
 *   index -> moving voxel coordinate, 12 doubles on the host).  Sample points: the fixed voxels (i, j, k) whose indices are all multiples
 *   of `stride`.  A sample is counted iff 0 <= p_a <= S_a - 1 on every axis (the overlap only: no zero padding enters) and both values
 *   are finite.  The fixed value is the stored voxel's; the moving value is mode 0 of mud_volume_regrid at p, so the histogram is that of
 *   (fixed, mud_volume_regrid(moving, m)) over the counted samples.  bin = clamp((int)floor((double(v) - lo) * scale), 0, bins - 1), the
 *   subtraction and the product rounded separately; hist[bin_fix][bin_mov] += 1.  hist: device, uint32 [bins][bins], cleared first
 *   (stream-ordered).  Counts are integers (LDS atomics per workgroup, one global atomic per non-empty bin): the result does not depend
 *   on the order of arrival and is the same bits on every run.  bins: 2 to 64; stride > 0; m, lo and scale finite.
 * mud_volume_mirror_moments (--align; no reference counterpart): what the search for a head's mid-sagittal plane
 *   evaluates: the moments of a stored volume (X x Y x Z) against its own mirror image through K candidate planes, in one launch.  mats:
 *   device, K x 12 doubles, 8-byte aligned; candidate k's 3 x 4 matrix (the matrix of mud_volume_regrid) maps a voxel index to the voxel
 *   coordinate p of its mirror image.  Sample points and the overlap rule are mud_volume_joint_hist's: the voxels whose indices are all
 *   multiples of `stride`; a pair is counted iff 0 <= p_a <= S_a - 1 on every axis and both values are finite; a = bin of the stored
 *   voxel's value, b = bin of mode 0 of mud_volume_regrid at p, both by mud_volume_joint_hist's formula with the one (lo, scale).
 *   sums: device, uint64 [K][6], 8-byte aligned, cleared first (stream-ordered): n, sum a, sum b, sum a^2, sum b^2, sum a b over the
 *   counted pairs of candidate k.  A candidate whose matrix holds a value that is not finite counts nothing (its p fails the overlap
 *   rule); the matrices are device memory and are not inspected on the host (mudiff_hip.ops.volume_mirror_moments refuses them before
 *   it uploads them).  Integer sums (registers, wave shuffles, LDS, then one 64-bit atomic add per workgroup, candidate and non-zero sum):
 *   the result does not depend on the order of arrival, nor on which other candidates share the launch, and is the same bits on every
 *   run.  bins: 2 to 256; stride > 0; 1 <= K <= 1048560; lo and scale finite.
 * mud_volume_bias_* (--bias_correct): the device's share of an N4-style bias-field correction; the loop around
 *   them is mudiff_hip.volume_bias.loop.  Sample points: the voxels whose indices are all multiples of `shrink`, nx x ny x nz of them (nx =
 *   ceil(X / shrink), ...), flat with x fastest.  The field F is a sum of uniform cubic B-spline lattices: level l = 0 .. levels - 1 (at
 *   most 5) has n = 2^l spans per axis and (n + 3)^3 fp64 control points [cz][cy][cx]; `lattices` holds the levels one after the other
 *   (device, 8-byte aligned).  On an axis of size S voxel i sits at x = (double(i) + 0.5) * double(n) / double(S), span = floor(x), t = x -
 *   span, with weights b0 = (1 - t)^3 / 6, b1 = (3 t^3 - 6 t^2 + 4) / 6, b2 = (3 t^2 - 3 t^3 + 3 t + 1) / 6, b3 = t^3 / 6 on the control
 *   points span .. span + 3; F = sum over levels, then over the 4 x 4 x 4 support (x fastest) of (bx * by) * bz * L.  Every fp64
 *   expression is evaluated uncontracted in the order of tests/volume_bias_ref.py.
 *   _log: u[sample] = logf(value of the stored voxel) where that value is finite and > 0 (the mask), NaN elsewhere.
 *   _corrected: c_new = float32(double(u) - F), NaN where u is; stats (device, 3 x uint64, cleared first): [0] the bits of the largest
 *     |double(c_new) - double(c_old)| that is a number (0 without any), [1] / [2] the order-preserving keys (an fp32's bits with the sign
 *     bit set for a positive value, all bits flipped for a negative one) of the largest / smallest finite c_new; [2] stays all ones without a
 *     finite sample.  c_new must not be u or c_old.
 *   _hist: hist[clamp((int)floor((double(c) - lo) * scale), 0, bins - 1)] += 1 over the finite c (mud_volume_joint_hist's formula);
 *     hist: device uint32 [bins], cleared first.  bins: 2 to 1024.
 *   _fit: one level's multilevel-B-spline sums of the residual r = double(c) - table(c) over the finite c; table: device fp64 [bins], the
 *     value at each bin centre, interpolated linearly in p = (double(c) - lo) * scale - 0.5 and clamped at the ends.  With w = (bx * by) * bz
 *     and S2 = (sum bx^2)(sum by^2)(sum bz^2) each control point of the support receives llrint(((w * w) * w) * r / S2 * 2^k) into
 *     sums[0][cp] (delta) and llrint((w * w) * 2^k) into sums[1][cp] (omega); sums: device int64 [2][(n + 3)^3], cleared first.  The caller
 *     picks k (0 .. 62) so that no sum can overflow (volume_bias.choose_k).  level: 0 .. 4 (a lattice of more than 16 spans does not fit in LDS).
 *   _apply: out (fp32 [Z][Y][X], 16-byte aligned, not vol) = float32(double(v) / exp(F)) at every voxel; a zero stays zero and a
 *     non-finite voxel is passed through.  With field != 0 out is float32(exp(F)) instead.
 *   Integer atomics only: every result is the same bits on every run.
 * mud_volume_denoise_* (--denoise; no reference counterpart): 3D non-local means of a stored volume and the
 *   estimate of its noise level; the host's share is mudiff_hip.volume_denoise.  v = the value of a stored voxel (fp32), valid iff finite.
 *   _residual (no reference counterpart): keys[i] (device uint32 [Z][Y][X]) = the bits of |eps|, eps = float32(sqrt(6 / 7)) *
 *     (v - (sum of the six face neighbours in the order -x +x -y +y -z +z, fp32) / 6), for the voxels that are > 0 and whose six face
 *     neighbours are inside the volume, valid and > 0; 0xFFFFFFFF for every other voxel.
 *   _select_hist (no reference counterpart): one pass (0 .. 3, most significant byte first) of a radix select over n keys:
 *     hist (device uint32 [256], cleared first)[byte 3 - pass of key] += 1 over the keys that are not 0xFFFFFFFF and whose `pass` higher
 *     bytes equal `prefix`.  The host picks the bin that holds the wanted rank and extends the prefix by it.
 *   _nlm (no reference counterpart): out (fp32 [Z][Y][X], not vol).  For every offset t != 0 with |t|_inf <= search, in z-outermost /
 *     x-fastest order, q = p + t is a candidate iff it is inside the volume and p and q are valid; d2 = (the fp32 sum over the patch offsets
 *     |o|_inf <= patch, z outermost and x fastest, of (v(p + o) - v(q + o))^2 where both voxels are inside and valid) / their number; w =
 *     expf(-(d2 / h)), h = float32(2 * beta * sigma * sigma); in fp64 sw += w, sa += w * a(q), a = double(v), or double(v)^2 with rician.
 *     m = (sa + wmax a(p)) / (sw + wmax), wmax the largest w, or 1 where that is not > 0 (no candidate); out = float32(m), or with rician
 *     float32(sqrt(max(m - 2 sigma^2, 0))).  A voxel that is 0 or not valid is passed through.  zeroed (device uint32, cleared first): the
 *     number of voxels that were not 0 and came out 0.  search: 1 .. 5, patch: 1 .. 2 (the tile and its halo of search + patch voxels per
 *     side are staged in LDS); sigma, beta: finite and > 0.  A fixed order of accumulation: the same bits on every run.
 * mud_volume_unring_* (--unring, DESIGN.md section 5.30, which holds the definition; no reference counterpart): removal of truncation (Gibbs)
 *   ringing by local sub-voxel shifts; the host's share (the tables) is mudiff_hip.volume_unring.  Axes are storage axes (0 = x, the
 *   fastest); every in-plane axis has at most 512 voxels; volumes are [Z][Y][X].
 *   _filter ("2D"): v = the value of a stored voxel, a non-finite one read as 0; nonfinite (device uint32, cleared first) counts
 *     them.  Per slice normal to the third axis, ix (fp32) = v circularly filtered by Gx(kx, ky) = cy / (cx + cy), c = 1 + cos(2 pi k / n)
 *     along axis_x and axis_y (1/2 at the bin 2 kx = nx, 2 ky = ny), and iy = v - ix.  twiddle: fp64 [nx][2] = (cos, -sin)(2 pi m / nx);
 *     kernel: fp64 [nx / 2 + 1][ny], row kx the inverse transform along ky of Gx(kx, .) (real).  ix and iy are also the workspace (the half
 *     spectrum along axis_x, fp32): buffers of their own.  Sums are fp64 chains in index order: the same bits on every run.
 *   _lines ("U(x)"): every line of `in` (fp32) along `axis`, circular: for the shifts s_j, j = 0 .. 2 shifts, y_s = the line
 *     convolved with row j of table (fp32 [2 shifts + 1][n], D_s of the definition; row 0 is not read: y_0 is the line), TV_s[l] = the
 *     smaller of the sums of |y_s[i] - y_s[i-1]| over the b - a + 1 differences that end a .. b voxels to the left of l and that begin a ..
 *     b voxels to its right; j* = the first j of the smallest TV_s[l]; the result is y_s[l] + |s| (y_s[l -+ 1] - y_s[l]) for s >< 0 and
 *     in[l] for j* = 0.  out = the result, or out + the result with accumulate != 0; out may be `in`.  jmap (int8, or NULL) = j*.  counters
 *     (device uint64 [2], cleared first): the voxels with j* != 0 and the sum of |s_j*| (2 shifts + 1).  `normal`, the slices' normal, only
 *     has to differ from `axis`: the lines of every slice are all the lines of the volume.  shifts: 1 .. 32; 1 <= a <= b <= 8; 2 b + 2
 *     <= n <= 512.  Fixed-order fp32 sums and integer counters: the same bits on every run.
 * mud_volume_fg_* (--foreground; no reference counterpart): a foreground (head or object) mask of a stored volume
 *   by thresholding and topology - not a brain extraction; the host's share (the Otsu scan) is mudiff_hip.volume_foreground.  v = the value
 *   of a stored voxel (fp32); a candidate is a voxel whose v is finite and != 0.  Masks are uint8 [Z][Y][X] holding 0 or 1, labels int32.
 *   _range: range (device uint32 [3], cleared first): with key(v) = bits | 0x80000000 for v >= 0 and ~bits for v < 0, [0] = the largest
 *     ~key (the smallest candidate), [1] = the largest key, [2] = the number of candidates; all 0 without one.
 *   _hist: hist (device uint32 [bins], cleared first)[bin(v)] += 1 over the candidates, bin = mud_volume_joint_hist's formula with lo and
 *     scale.  bins: 16 to 1024; lo finite; scale finite and > 0.
 *   _mask: mask[i] = 1 iff i is a candidate and bin(v) > k, else 0.  k: 0 .. bins - 2.
 *   _morph: one erosion (dilate 0: on iff the voxel and its six face neighbours are on, a neighbour outside the volume counts as on) or
 *     one dilation (dilate 1: on iff any of the seven is on, outside counts as off) from `in` to `out` (not in place).
 *   _label: the 6-connected components of the voxels whose mask is `value` (1: on, 0: off): labels[i] = the smallest linear index (x
 *     fastest) of i's component, -1 for every other voxel.  A block-based union-find in three launches (tile-local in LDS, tile faces by a
 *     lock-free union, path compression); no launch count and no loop depends on the data beyond the depth of a tree.
 *   _census: census (device uint32 [X*Y*Z], cleared first)[root] = the component's voxel count, with bit 31 set iff one of its voxels lies
 *     on a face of the volume; summary (device uint64 [2], cleared first): [0] = the largest (count << 32) | (0xFFFFFFFF - root), i.e. the
 *     largest component, the smallest root on a tie; [1] = the number of components.
 *   _select: holes 0: mask[i] = (labels[i] == root); holes 1: mask[i] = 1 wherever labels[i] >= 0 and census[labels[i]] has bit 31 clear
 *     (the rest of the mask stays).  count (device uint32, cleared first): the voxels switched on.
 *   _apply: out (fp32 [Z][Y][X], not vol)[i] = v where mask[i] != 0 (its bits as they are, a NaN included), +0 elsewhere; removed (device
 *     uint32, cleared first): the candidates outside the mask.
 *   X*Y*Z < 2^31.  Integer atomics only: every result is the same bits on every run.
 * mud_volume_edt* (--brain_extract; no reference counterpart): morphology by a radius in millimetres on an
 *   anisotropic grid, as a threshold on an exact Euclidean distance transform; the host's share (a morphological estimate of the brain -
 *   not a learned extraction) is mudiff_hip.volume_brain.  Masks are uint8 [Z][Y][X] holding 0 or 1, as above.
 *   _edt: d2 (fp64 [Z][Y][X], 16-byte aligned)[p] = the squared distance, in the units of sx, sy, sz, from voxel p to the nearest voxel
 *     of the volume whose mask equals `value` (0 or 1): 0 at such a voxel, +inf everywhere without one.  Voxels outside the volume do not
 *     exist: they count as neither on nor off.  Bit for bit: with wx = sx * sx, wy = sy * sy, wz = sz * sz (each rounded once) and the
 *     integer offsets (dx, dy, dz) to a voxel q, every product and sum rounded separately,
 *         d2[p] = min over q of ((wx * (dx * dx)) + (wy * (dy * dy))) + (wz * (dz * dz)).
 *     fp64 addition is monotone, so this is three passes of out(i) = min over j of (in(j) + w * ((i - j) * (i - j))) along x, y and z
 *     (one kernel, the lines staged in LDS, each scan pruned once w * k^2 is not below the best so far).  sx, sy, sz: finite and > 0; no
 *     axis longer than 1024 voxels (a line is staged whole).
 *   _edt_select: out[i] = (above ? d2[i] > r2 : d2[i] <= r2) && (within == NULL || within[i] != 0), over n voxels; count (device uint32,
 *     cleared first): the voxels switched on.  r2: finite and >= 0; above: 0 or 1; out is not within.
 *   X*Y*Z < 2^31.  No floating-point atomics: every result is the same bits on every run.
 *
 * mud_volume_reorient (--reorient; replaces nibabel's as_closest_canonical / apply_orientation, which the
 *   reference does not call: it reads its files unreoriented): a permutation and flips of the storage axes of a volume of
 *   elem_bytes-wide elements (1, 2, 4 or 8: every stored datatype, fp32 and fp64; the values are moved, never interpreted), x fastest on
 *   both sides.  With S = (SX, SY, SZ), p = (p0, p1, p2) a permutation of (0, 1, 2) and flip_o = bit o of flip_mask, the destination has
 *   the extents (S[p0], S[p1], S[p2]) and dst[i0, i1, i2] = src[j], j[p_o] = flip_o ? S[p_o] - 1 - i_o : i_o.  p0 == 0 copies whole
 *   x-rows (backwards under flip_0); otherwise tiles of the plane (source x, source axis p0) go through LDS, read in runs along source x
 *   and written in runs along destination x.  MUD_ERR_ARG before any launch for an elem_bytes outside {1, 2, 4, 8}, a p that is not a
 *   permutation, a flip_mask outside [0, 7], a negative extent, SX*SY*SZ >= 2^31, a null or misaligned pointer and a source that overlaps
 *   the destination (src == dst included: not an in-place operation).  A volume without voxels launches nothing and succeeds.
 * mud_volume_lowpass (--antialias / --conform; what scipy.ndimage.gaussian_filter1d does before a zoom below 1,
 *   which the reference never performs: it takes its volumes on the training grid): a separable Gaussian low-pass of a stored volume in
 *   front of a resampling that downsamples.  wx / wy / wz: HOST arrays of 2 r + 1 weights w[t + r], t = -r..r, computed by the caller in
 *   fp64 (mudiff_hip.volume_conform.weights); a null array skips that axis.  The passes run in x, y, z order; one pass along axis a is
 *   out[i] = (sum_t w[t] v[i + t]) / (sum_t w[t]), both sums over the t with 0 <= i + t < S_a, t ascending (truncation with
 *   renormalisation), products and sums in fp64, rounded to fp32 once.  v is the value of the stored voxel (datatype, slope, inter as
 *   everywhere) on the first pass that runs and the fp32 of the pass before on the later ones; a non-finite value is read as 0, and
 *   *nonfinite (device, cleared first) counts those of the stored volume.  out: fp32 [Z,Y,X], what mud_volume_regrid reads as an
 *   MUD_NIFTI_F4 source of slope 1; scratch: a second fp32 [Z,Y,X] volume, needed (and touched) only when two or three axes are
 *   filtered.  Every global access runs along x: the x pass stages a row segment and its halo in LDS, the y and z passes an x-run times
 *   a stretch of the filtered axis.  With all three arrays null nothing is launched and nothing is written.  MUD_ERR_ARG before any
 *   launch for a radius outside [0, 16], a weight that is not finite or negative, a centre weight of 0, an unsupported datatype, a bad
 *   size, a null or misaligned pointer, and an output that overlaps the source or the scratch volume. */
#define MUD_NIFTI_U1 2
#define MUD_NIFTI_I2 4
#define MUD_NIFTI_I4 8
#define MUD_NIFTI_F4 16
#define MUD_NIFTI_U2 512
#define MUD_VI_MAX_RANKS 4
#define MUD_VI_WINDOW 16
typedef struct mud_volume_census_record {
  uint64_t n, n_nonfinite;
  float min, max;
  int32_t count[MUD_VI_MAX_RANKS];
  int64_t first_rank[MUD_VI_MAX_RANKS];
  float window[MUD_VI_MAX_RANKS][MUD_VI_WINDOW];
} mud_volume_census_record;
int64_t mud_volume_census_ws_bytes(void);
int mud_volume_census(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* q, int nq,
                      mud_volume_census_record* record, void* ws, int64_t ws_bytes, void* stream);
int mud_volume_slab_normalise(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, float lo, float den,
                              int degenerate, int s0, int s1, float* out, void* stream);
int mud_volume_slab_zscore(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, float mean, float std, int s0,
                           int s1, float* out, void* stream);
int mud_volume_assemble(const float* planes, const float* planes2, int X, int Y, int Z, int s0, int s1, float* vol, float* vol2,
                        void* stream);
int mud_volume_regrid(const void* src, int datatype, int SX, int SY, int SZ, float slope, float inter, const double* m, int mode, int X,
                      int Y, int Z, float* out, void* stream);
int mud_volume_bspline_coeffs(const void* vol, int datatype, int SX, int SY, int SZ, float slope, float inter, double* coeffs,
                              uint32_t* nonfinite, void* stream);
int mud_volume_regrid_cubic(const double* coeffs, int SX, int SY, int SZ, const void* src, int datatype, float slope, float inter,
                            const double* m, double lo, double hi, int X, int Y, int Z, float* out, void* stream);
int mud_volume_joint_hist(const void* fix, int fix_dt, int X, int Y, int Z, float fix_slope, float fix_inter, const void* mov, int mov_dt,
                          int SX, int SY, int SZ, float mov_slope, float mov_inter, const double* m, int stride, double fix_lo,
                          double fix_scale, double mov_lo, double mov_scale, int bins, uint32_t* hist, void* stream);
int mud_volume_mirror_moments(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* mats, int K,
                              int stride, double lo, double scale, int bins, uint64_t* sums, void* stream);
int mud_volume_bias_log(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, int shrink, float* u, void* stream);
int mud_volume_bias_corrected(const float* u, const float* c_old, float* c_new, const double* lattices, int levels, int X, int Y, int Z,
                              int shrink, uint64_t* stats, void* stream);
int mud_volume_bias_hist(const float* c, int64_t n, double lo, double scale, int bins, uint32_t* hist, void* stream);
int mud_volume_bias_fit(const float* c, const double* table, int bins, double lo, double scale, int level, int X, int Y, int Z, int shrink,
                        int k, int64_t* sums, void* stream);
int mud_volume_bias_apply(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* lattices, int levels,
                          int field, float* out, void* stream);
int mud_volume_denoise_residual(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, uint32_t* keys, void* stream);
int mud_volume_denoise_select_hist(const uint32_t* keys, int64_t n, uint32_t prefix, int pass, uint32_t* hist, void* stream);
int mud_volume_denoise_nlm(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, int search, int patch, double sigma,
                           double beta, int rician, float* out, uint32_t* zeroed, void* stream);
int mud_volume_unring_filter(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, int axis_x, int axis_y,
                             const double* twiddle, const double* kernel, float* ix, float* iy, uint32_t* nonfinite, void* stream);
int mud_volume_unring_lines(const float* in, int X, int Y, int Z, int axis, int normal, int shifts, int a, int b, const float* table,
                            float* out, int accumulate, int8_t* jmap, uint64_t* counters, void* stream);
int mud_volume_fg_range(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, uint32_t* range, void* stream);
int mud_volume_fg_hist(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, double lo, double scale, int bins,
                       uint32_t* hist, void* stream);
int mud_volume_fg_mask(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, double lo, double scale, int bins, int k,
                       uint8_t* mask, void* stream);
int mud_volume_fg_morph(const uint8_t* in, int X, int Y, int Z, int dilate, uint8_t* out, void* stream);
int mud_volume_fg_label(const uint8_t* mask, int X, int Y, int Z, int value, int32_t* labels, void* stream);
int mud_volume_fg_census(const int32_t* labels, int X, int Y, int Z, uint32_t* census, uint64_t* summary, void* stream);
int mud_volume_fg_select(const int32_t* labels, const uint32_t* census, int64_t n, int root, int holes, uint8_t* mask, uint32_t* count,
                         void* stream);
int mud_volume_fg_apply(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const uint8_t* mask, float* out,
                        uint32_t* removed, void* stream);
int mud_volume_edt(const uint8_t* mask, int X, int Y, int Z, int value, double sx, double sy, double sz, double* d2, void* stream);
int mud_volume_edt_select(const double* d2, int64_t n, double r2, int above, const uint8_t* within, uint8_t* out, uint32_t* count,
                          void* stream);
int mud_volume_reorient(const void* src, int elem_bytes, int SX, int SY, int SZ, int p0, int p1, int p2, int flip_mask, void* dst,
                        void* stream);
int mud_volume_lowpass(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* wx, int rx,
                       const double* wy, int ry, const double* wz, int rz, float* out, float* scratch, uint32_t* nonfinite, void* stream);

#ifdef __cplusplus
}
#endif
#endif
