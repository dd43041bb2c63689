/* saltnet.h — C-ABI of the MI355X-native U-Net hot path (libsaltnet_hip.so, gfx950).
 *
 * The reference (neptune-ai/open-solution-salt-identification) is pure Python on PyTorch; the
 * arithmetic this library replaces is reached from it through torch operator calls inside the
 * nn.Module classes cited next to each entry point (paths relative to the reference's
 * common_blocks/).  A maintainer binds these symbols with ctypes; there are no
 * torch types in any signature: plain pointers to device memory, sizes and a HIP stream.
 *
 * Conventions
 *   - Every operator is `int salt_<op>(const salt_<op>_args*, void* stream)`; 0 = success,
 *     otherwise a SALT_E_* code or a hipError_t (> 0).  `stream` is a hipStream_t (NULL = default).
 *   - The library never allocates or frees device memory; workspaces are passed in.
 *   - Activations are NHWC, element type given by `dtype` (SALT_F32 / SALT_BF16).  A `salt_view`
 *     describes a [B,H,W,C] tensor whose pixels are `cs` elements apart (cs >= C), so a channel
 *     slice of a wider buffer (a "concat-free" skip connection) is a view, not a copy.
 *   - Parameters, gradients, statistics and losses are fp32.
 *   - This header is parsed by the Python host (salt_amd/_abi.py) to build the ctypes structures:
 *     keep one field per line, only the scalar/array/view forms used below.
 */
#ifndef SALTNET_H
#define SALTNET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALT_F32 0
#define SALT_BF16 1

#define SALT_OK 0
#define SALT_E_BADARG -1
#define SALT_E_UNSUPPORTED -2
#define SALT_E_LDS -3

#define SALT_MAX_TAPS 16

typedef struct {
    void* p;      /* device pointer to element [0,0,0,0] of the view */
    int B;
    int H;
    int W;
    int C;        /* channels in the view */
    int cs;       /* pixel stride in elements */
} salt_view;

/* ------------------------------------------------------------------ library / device info */
int salt_abi_version(void);                 /* bumps when any struct below changes */
int salt_device_info(int* cu_count, int* lds_bytes, char* arch_name, int arch_name_len);
int salt_abi_struct_sizes(int* out, int n); /* sizeof of every struct below, declaration order */
const char* salt_last_error(void);          /* text for the last non-zero return on this thread */

/* ------------------------------------------------------------------ implicit-GEMM convolution
 * One kernel family serves nn.Conv2d 3x3/1x1 (stride 1|2, zero pad: unet_models.py:24, torchvision
 * BasicBlock/Bottleneck; replicate pad top/right: architectures/base.py:21-27), one output-parity
 * phase of nn.ConvTranspose2d k3/k4 s2 (unet_models.py:44,60; base.py:48-49), and their
 * data-gradients (same kernel, transposed packed weights, mirrored taps).
 *   out[b, oy*out_step+out_oy, ox*out_step+out_ox, n] (+)= epi( sum_t sum_c
 *        X[b, pad(oy*in_step + tap_dy[t]), pad(ox*in_step + tap_dx[t]), c] * Wp[t][n][c] )
 *   epi(v) = relu?( (v + bias[n]) * scale[n] + shift[n] )        (each part optional; + res before the ReLU: see `res` below)
 * Wp is the packed layout produced by salt_pack_conv_weight: [ceil(Cin/KC)][ntaps][Cout][KC],
 * KC = 64 bytes of channels (16 f32 / 32 bf16), zero padded.
 * stats (optional): per output-tile-wave partial (sum, M2 about the partial's own mean, count) of
 * the stored value per channel, for train-mode BatchNorm (deterministic: no atomics).
 */
typedef struct {
    int dtype;
    salt_view x;
    const void* w;            /* packed weights */
    int ntaps;
    int tap_dy[SALT_MAX_TAPS];
    int tap_dx[SALT_MAX_TAPS];
    int in_step;              /* 1 | 2 */
    int pad_mode;             /* 0 zero, 1 clamp (replicate) */
    salt_view y;              /* FULL output buffer view [B,OHf,OWf,Cout] */
    int OH;                   /* logical output grid of this launch */
    int OW;
    int out_step;             /* 1 | 2 */
    int out_oy;
    int out_ox;
    const float* bias;        /* [Cout] or NULL */
    const float* scale;       /* [Cout] or NULL */
    const float* shift;       /* [Cout] or NULL */
    int relu;
    int accumulate;           /* y += result */
    float* stats;             /* [nparts][2][Cout] or NULL */
    float* stats_cnt;         /* [nparts] */
    int stats_part0;          /* first partial index written by this launch (ConvT phases) */
    int cfg;                  /* low byte: 0 = auto, else tile-config / kernel id (tests / tuning; salt_conv_kernel_id); (cfg >> 8) & 0xff:
                               * cap on the workgroups per XCD of conv_ws_kernel / conv_ls_kernel (0 = one per CU), whatever the low byte */
    /* Fold mode (data-gradient of a replicate-padded convolution, architectures/base.py:21-27): the launch computes the gradient on
     * the extended grid OH = y.H + fold_top + fold_bottom, OW = y.W + fold_left + fold_right; interior pixels go straight to y
     * (the UNPADDED tensor, (+)= per `accumulate`), the pad ring goes to `strip` ([B][salt_fold_strip_pixels][strip_cs], always
     * overwritten) and salt_pad_fold_strip adds the ring onto the edge pixels of y.
     * strip == NULL with fold_top > 0 or fold_right > 0 (fold_bottom = fold_left = 0): FUSED fold - same extended grid, but the launch
     * lays its tiles out so that every ring pixel shares a tile with the edge pixel it folds onto and the epilogue adds them before the
     * store: no strip, no second pass (needs out_step 1, no stats, 16-byte aligned y with C and cs multiples of 8 (bf16) / 4 (f32)).
     * strip == NULL and all pads 0: normal mode. */
    void* strip;
    int strip_cs;
    int fold_top;
    int fold_bottom;
    int fold_left;
    int fold_right;
    /* BatchNorm-backward sums fused into a data-gradient launch (the launch that completes g = dL/da of a = relu?(bn(yc)), yc the
     * producer convolution's output): each workgroup also reduces, over its pixel tile and per channel, sum(g m) and
     * sum(g m xhat) with m = [yc*scale + shift > 0] (or [a > 0] / 1, see bnb_a / bnb_relu), xhat = (yc - mean) invstd, of the value it STORES, into
     * bnb_partials[tile][2][Cout], tile < salt_conv_stats_parts(args).  salt_bn_bwd then runs with partials_ready = 1 and skips
     * its own reduction pass over g and yc.  bnb_partials == NULL: off.  Needs out_step 1 on the full grid, no strip, no stats,
     * 16-byte aligned views with Cout a multiple of 8 (bf16) / 4 (f32). */
    salt_view bnb_y;          /* yc, same shape as y */
    salt_view bnb_a;          /* residual layers, a = relu(bn(yc) + res): the forward output the mask comes from (m = [a > 0]); p == NULL: mask from yc */
    const float* bnb_mean;
    const float* bnb_invstd;
    const float* bnb_gamma;
    const float* bnb_beta;
    float* bnb_partials;
    int bnb_relu;
    /* Phase-fused stride-2 launch (nphase == 4): the four output-parity phases of a transposed convolution / stride-2 data gradient in
     * ONE launch.  Every phase runs the same `ntaps` tap offsets over x and writes y at (2 oy + ay, 2 ox + ax), phase = 2 ay + ax
     * (out_oy / out_ox are ignored, out_step must be 2, OH x OW is the per-phase grid); phase p reads the packed weights at
     * w + p * w_phase_elems elements (taps a phase does not have are packed as zeros: tap_kh < 0 in salt_pack_conv_weight).  BN
     * statistics partials are numbered over all phases.  nphase <= 1: a plain launch. */
    int nphase;
    int64_t w_phase_elems;
    /* In-launch BatchNorm finalize.  fin != NULL (a const salt_bn_finalize_args*, declared below; its stats / stats_cnt / nparts are
     * ignored): the launch accumulates its per-tile (sum, sum of squares, count) into fin_acc with fp64 atomics - 8 shards
     * [8][2 * Cout + 1] doubles, shard = workgroup id % 8 (one per XCD), summed in shard order - takes a ticket on fin_ticket, and the
     * workgroup that arrives last computes what salt_bn_finalize would have (mean / invstd / scale / shift, running statistics) before
     * the launch ends: no partials round trip, no separate launch.  `stats` must be NULL.  fin_acc and fin_ticket must be zero before
     * the first launch; every launch leaves them zero.  One launch per BatchNorm layer (no stats_part0 chaining).  The fp64 sums are
     * order dependent in their last bits only (the fp32 results are reproducible in practice, not by construction).
     * bnb_fin != NULL (a const salt_bn_bwd_args*): the same for the BatchNorm-backward sums of bnb_*: the last workgroup writes
     * dgamma / dbeta / coef, and salt_bn_bwd then runs with partials_ready = 2 (apply pass only).  bnb_partials is ignored (may be NULL).
     * fin_ticket == NULL with fin_acc != NULL (bnb_ticket == NULL with bnb_acc != NULL): the launch only ADDS to the shards - no wait,
     * no ticket, fin / bnb_fin unused - and the consumer finalizes them (salt_affine_act_args.fin_acc; salt_bn_bwd with
     * partials_ready = 3).  The shards must then be cleared by the caller before the next launch (one salt_zero over all layers). */
    const void* fin;
    double* fin_acc;
    uint32_t* fin_ticket;
    const void* bnb_fin;
    double* bnb_acc;          /* [8][2 * Cout] */
    uint32_t* bnb_ticket;
    /* Residual epilogue (eval-mode torchvision BasicBlock / Bottleneck, out = relu(bn(conv(a)) + identity), architectures/encoders.py:6-45):
     * res.p != NULL: y = relu?( round_to_dtype((v + bias) * scale + shift) + res ), res a [B,OH,OW,Cout] view - the values a separate
     * salt_affine_act(y, res, relu) pass over the stored convolution output would produce, bit for bit, without that pass.  Plain
     * full-grid launches only (out_step 1, no fold / strip / statistics / accumulate). */
    salt_view res;
    /* Input transform: the PRODUCER's BatchNorm apply + ReLU folded into this launch's loader (the measured alternative to the
     * separate salt_affine_act pass between a convolution and its single consumer, architectures/base.py:29-37, unet_models.py:21-30;
     * DESIGN 10 has the numbers).  in_scale != NULL or in_fin_acc != NULL: every in-range input element becomes
     * x' = round_to_dtype(relu?(x * in_scale[c] + in_shift[c])) - the value salt_affine_act would have stored - between the global
     * load and the LDS store; zero padding stays zero.  in_fin_acc: the [8][2 Cin + 1] fp64 shards of the producer's statistics
     * (salt_conv_args.fin_acc without a ticket) are finalized in every workgroup's prologue with in_fin (the producer layer's const
     * salt_bn_finalize_args*), workgroup 0 stores mean / invstd / scale / shift / running statistics: in_scale / in_shift are ignored.
     * bf16, 9 taps, whole aligned 16-byte pieces; runs on conv_mfma_kernel's register-staged loader (never the LDS-DMA kernels). */
    const float* in_scale;    /* [Cin] */
    const float* in_shift;
    int in_relu;
    const void* in_fin;
    const double* in_fin_acc;
    /* Planar y: y_plane != 0 (elements): y is stored as C / y.cs dense planes [B,H,W,y.cs] - channel c of pixel q at
     * y.p + (c / y.cs) * y_plane + q * y.cs + c % y.cs - instead of channel-interleaved rows (y.cs < y.C is legal only here).  The
     * gradient of the 320-channel hypercolumn (architectures/unet.py:101-107) is kept this way: the five consumers (the up-sampling
     * adjoints, the scSE backward of dec1) each read ONE dense 64-channel plane instead of 128-byte pieces at a 640-byte pitch.
     * conv_ws_kernel only (y.cs == 64 = its channel block); salt_conv fails for any other launch, salt_conv_kernel_id returns -1. */
    int64_t y_plane;
    /* Planar x, the same layout on the input side: channel c of pixel q at x.p + (c / x.cs) * x_plane + q * x.cs + c % x.cs.  The
     * forward convolution over the hypercolumn reads its 32-channel chunks from the five level planes.  conv_ls_kernel only
     * (x.cs == 64: two chunks per plane). */
    int64_t x_plane;
} salt_conv_args;
int salt_conv(const salt_conv_args*, void* stream);
/* number of stats partials a launch with these args writes (host sizes the workspace with it) */
int salt_conv_stats_parts(const salt_conv_args*);
/* which kernel salt_conv runs these arguments on: 1..5 conv_mfma_kernel tile configs, 6..8 conv_glds_kernel, 9 conv_ws_kernel (the
 * weight-stationary multi-tile kernel of the 3x3 layers with <= 64 channels: bf16, Cin in {32, 64}, Cout in {32, 64}, output grid a
 * multiple of 16 x 16), 10 conv_ls_kernel (the loader-specialised streaming kernel of the deeper 3x3 layers: bf16, Cin >= 64 and Cout
 * multiples of 32, same grid rule), 11 conv1x1_ls_kernel (the streaming kernel of the 1x1 convolutions with eval / plain epilogues
 * or train-mode statistics through fin_acc: bf16, Cin a multiple of 64, Cout of 32, B OH OW a multiple of 256; stride 1, or stride 2
 * on 16 x 16 output tiles), 12 conv_thin_kernel (the persistent weight-stationary kernel of the fp32 3x3 layers with 16 or 32
 * channels on BOTH sides, unit steps, output grid a multiple of 16 x 16; statistics / BatchNorm-backward sums through the fp64 shards
 * only), 13 conv_stem16_kernel (the ResNet stem after the 2 x 2 space-to-depth: bf16, 16 taps over 16 input channels -> 64, zero
 * padding, eval epilogue or train-mode statistics through fin_acc).  `cfg` & 0xff:
 * 0 = heuristic, 1..8 = that config, 9 .. 13 = that kernel wherever it applies (else heuristic); (cfg >> 8) & 0xff caps the
 * workgroups per XCD of kernels 9 - 11 (0 = one per CU) and, for 10 / 11 when asked for, (cfg >> 16) & 3 fixes the output channels
 * per item to 32 x that (0 = by size).  Asked-for variants of those two kernels (tests / A-B; round 5): kernel 11 - bit 18 the item-major
 * walk, bit 19 conv1x1_xs_kernel (input tile resident in LDS); kernel 10 - bit 20 two-tile items, bit 21 single tiles only. */
int salt_conv_kernel_id(const salt_conv_args*);
/* pixel tile of conv_mfma_kernel / conv_glds_kernel for these arguments (tests / tuning): tw | th << 8 | images << 16 | general << 24.
 * general = 1: a full-width strip of the extended grid of a fused-fold data gradient (th rows of tw = OW columns, or whole images)
 * instead of a power-of-two tile - the 10 / 18 / 34-wide grids of the decoder's replicate-padded layers fill 16-wide tiles to 40 - 60 %. */
int salt_conv_tile_shape(const salt_conv_args*);

/* weight gradient of the same family:
 *   dW[t][a][b] = sum_{pixels p of P} P[p, a] * Q[pad(p*q_step + tap[t]), b]
 * conv:  P = dY (a = cout), Q = X (b = cin);   convT: P = X (a = cin), Q = dY (b = cout).
 * Writes nsplit partial slabs [nsplit][ntaps][Ca][Cb] fp32 into `partials`;
 * salt_wgrad_reduce sums them in fixed order into the reference parameter layout. */
typedef struct {
    int dtype;
    salt_view p;
    salt_view q;
    int ntaps;
    int tap_dy[SALT_MAX_TAPS];
    int tap_dx[SALT_MAX_TAPS];
    int q_step;
    int pad_mode;
    float* partials;
    int nsplit;               /* as returned by salt_conv_wgrad_nsplit */
    int64_t q_plane;          /* != 0: q is planar (salt_conv_args.y_plane layout), q.cs == 64 = the kernels' b-block: block bb reads plane bb */
} salt_conv_wgrad_args;
int salt_conv_wgrad(const salt_conv_wgrad_args*, void* stream);
int salt_conv_wgrad_nsplit(const salt_conv_wgrad_args*);
/* which kernel family salt_conv_wgrad runs these arguments on (bench.py: roofline.kernel_symbol): 1 conv_wgrad_ls_kernel, 2
 * conv_wgrad_thin_kernel, 3 conv_wgrad_fast_kernel / fast8, 4 conv_wgrad_fast32_kernel, 5 conv_wgrad_kernel (generic); < 0: no plan */
int salt_conv_wgrad_kernel_id(const salt_conv_wgrad_args*);

typedef struct {
    const float* partials;    /* [nsplit][ntaps][Ca][Cb] */
    int nsplit;
    int ntaps;
    int Ca;
    int Cb;
    int KH;                   /* reference weight tensor is [Ca][Cb][KH][KW] */
    int KW;
    int tap_kh[SALT_MAX_TAPS];
    int tap_kw[SALT_MAX_TAPS];
    float* grad;              /* fp32, reference layout */
    int accumulate;
    int ldb;                  /* > 0: `grad` points at channel b = 0 of a SLICE of a wider [Ca][ldb][KH][KW] tensor (row stride of the Cb axis); 0: Cb */
    int a_mod;                /* > 0: "tap GEMM" slab (ntaps must be 1): slab row a = t * a_mod + a' is tap (tap_kh[t], tap_kw[t]) of reference row a';
                               * Ca / a_mod <= SALT_MAX_TAPS.  The factored hypercolumn (salt_hyper_stencil) computes the 3x3 weights of a level this way */
} salt_wgrad_reduce_args;
int salt_wgrad_reduce(const salt_wgrad_reduce_args*, void* stream);

/* fp32 master weight (reference layout) -> packed compute layout.
 * transpose=0: Wp[chunk][t][n=d0][c=d1]  from W[d0][d1][kh][kw]   (conv forward; convT dgrad)
 * transpose=1: Wp[chunk][t][n=d1][c=d0]                           (conv dgrad;   convT forward) */
typedef struct {
    int dtype;                /* of the packed copy */
    const float* w;           /* [D0][D1][KH][KW] */
    int D0;
    int D1;
    int KH;
    int KW;
    int ntaps;
    int tap_kh[SALT_MAX_TAPS];   /* < 0: a zero tap (phase-fused launches) */
    int tap_kw[SALT_MAX_TAPS];
    int transpose;
    void* wp;
    /* Sub-blocks (all 0: the whole tensor, as before).  d1_cnt > 0: only d1 in [0, d1_cnt) is packed - `w` points at the first channel of
     * a slice of the D1 axis, D1 stays the row stride.  n_off / n_total / chunk_off place the job inside a WIDER packed tensor: packed row
     * n + n_off of n_total rows (0: the job's own count), channel chunk + chunk_off.  The "tap GEMM" of the factored hypercolumn packs
     * the nine [Cout][Cin] tap matrices of a level as ONE 1x1 weight with 9 Cout output channels (forward: n_off = t Cout) and its
     * transpose with 9 Cout input channels (chunk_off = t Cout / KC). */
    int d1_cnt;
    int n_off;
    int n_total;
    int chunk_off;
} salt_pack_conv_weight_args;
int salt_pack_conv_weight(const salt_pack_conv_weight_args*, void* stream);
int64_t salt_packed_weight_elems(int dtype, int ntaps, int n, int c);

/* All pack jobs of a network in ONE launch: `jobs` is a DEVICE array of salt_pack_conv_weight_args (same dtype),
 * `job_block0` a DEVICE array [njobs+1] of prefix block counts (256 elements of the packed copy per block... see
 * salt_pack_job_blocks).  Replaces ~100 tiny launches per optimizer step by one. */
typedef struct {
    const void* jobs;
    const int* job_block0;
    int njobs;
    int total_blocks;
    int dtype;
} salt_pack_batched_args;
int salt_pack_batched(const salt_pack_batched_args*, void* stream);
int salt_pack_job_blocks(const salt_pack_conv_weight_args*);

/* ------------------------------------------------------------------ thin-channel direct convolutions
 * First layer (Cin <= 4: ResNet stem conv7x7 s2 p3, encoders.py:23-31 / torchvision; vanilla U-Net's
 * first 3x3) and heads with Cout <= 4 (final 1x1 unet.py:84-87, unet_models.py:138; sSE base.py:110).
 * These are not dense contractions; they run on the vector ALUs. */
typedef struct {
    int dtype;                /* dtype of y */
    const float* x;           /* input image batch, fp32 NCHW [B,Cin,H,W] (the reference batch contract) */
    int B;
    int Cin;
    int H;
    int W;
    const float* w;           /* fp32 master weight [Cout][Cin][K][K] */
    int K;
    int stride;
    int pad;                  /* zero padding */
    salt_view y;              /* [B,OH,OW,Cout] */
    const float* bias;
    const float* scale;
    const float* shift;
    int relu;
    float* stats;             /* NULL or [tiles][2][Cout] fp32, tiles = salt_conv_first_stats_parts: per 16 x 16 output tile (image-major, then tile row,
                               * tile column) the sum over the tile's pixels inside the image, then M2 = sum (v - tile mean)^2 of the same pixels;
                               * v is the epilogue value before its storage rounding (the salt_bn_finalize partial layout) */
    float* stats_cnt;         /* [tiles] fp32: the tile's count of pixels inside the image (required with stats) */
} salt_conv_first_args;
int salt_conv_first(const salt_conv_first_args*, void* stream);
int salt_conv_first_stats_parts(const salt_conv_first_args*);

typedef struct {
    int dtype;                /* dtype of dy */
    const float* x;
    int B;
    int Cin;
    int H;
    int W;
    int K;
    int stride;
    int pad;
    salt_view dy;
    float* partials;          /* [nparts][Cout*Cin*K*K] */
    int nparts;               /* as returned by salt_conv_first_wgrad_parts */
    float* grad;              /* [Cout][Cin][K][K] */
    int accumulate;
} salt_conv_first_wgrad_args;
int salt_conv_first_wgrad(const salt_conv_first_wgrad_args*, void* stream);
int salt_conv_first_wgrad_parts(const salt_conv_first_wgrad_args*);
/* which instantiation salt_conv_first_wgrad runs these arguments on (host only, no launch; tests): low byte 0 = the MFMA path of
 * conv_first_wgrad_kernel (Cout % 16 == 0, K K Cin <= 16), else its scalar loop's PER (1, 4, 12 or 40 taps per thread); + 256 when
 * partial_sum_wide_kernel reduces the partials (nparts >= 64 and Cout Cin K K <= 4096), else partial_sum_kernel; < 0: refused */
int salt_conv_first_wgrad_kernel_id(const salt_conv_first_wgrad_args*);

/* ResNet stem on the matrix cores: conv KxK stride 2 (K odd, pad K/2; 7x7 s2 p3 in torchvision) over Cin <= 4 channels
 * == a ((K+1)/2)^2-tap stride-1 convolution over the 2x2 space-to-depth image z[b,Y,X,(ph*2+pw)*Cin+c] = x[b,c,2Y+ph,2X+pw]
 * (4*Cin channels zero-padded to 16).  These three helpers move data / weights / weight-gradients between the two forms;
 * the convolution itself and its weight gradient are salt_conv / salt_conv_wgrad on z. */
typedef struct {
    int dtype;
    const float* x;           /* fp32 NCHW [B,Cin,H,W], H and W even */
    int B;
    int Cin;
    int H;
    int W;
    salt_view z;              /* [B,H/2,W/2,16] */
} salt_s2d_args;
int salt_s2d(const salt_s2d_args*, void* stream);

typedef struct {
    int dtype;                /* of the packed copy */
    const float* w;           /* [Cout][Cin][K][K] fp32 master */
    int Cout;
    int Cin;
    int K;
    void* wp;                 /* packed [1][T*T][Cout][KC], T = (K+1)/2, tap t = (dh+T/2)*T + (dw+T/2) */
} salt_pack_stem_weight_args;
int salt_pack_stem_weight(const salt_pack_stem_weight_args*, void* stream);

typedef struct {
    const float* g16;         /* [Cout][16][T][T] fp32: weight gradient in the space-to-depth form */
    int Cout;
    int Cin;
    int K;
    float* grad;              /* [Cout][Cin][K][K] */
    int accumulate;
} salt_stem_grad_unfold_args;
int salt_stem_grad_unfold(const salt_stem_grad_unfold_args*, void* stream);

typedef struct {
    int dtype;
    salt_view x;
    const float* w;           /* [Cout][Cin] fp32, Cout <= 4 */
    const float* bias;        /* [Cout] or NULL */
    int Cout;
    float* y_nchw;            /* fp32 [B,Cout,H,W] or NULL */
    salt_view y;              /* NHWC output (used when y_nchw == NULL) */
} salt_head1x1_args;
int salt_head1x1(const salt_head1x1_args*, void* stream);
/* which kernel salt_head1x1 runs these arguments on (host only, no launch; tests): 1 head1x1_kernel (scalar), 2 head1x1_vec_kernel,
 * 3 head1x1_vec_co_kernel<2>; < 0: refused */
int salt_head1x1_kernel_id(const salt_head1x1_args*);

typedef struct {
    int dtype;
    salt_view x;
    const float* w;
    int Cout;
    const float* dy_nchw;     /* fp32 [B,Cout,H,W] */
    salt_view dx;             /* grad wrt x */
    int accumulate;
    float* partials;          /* [nparts][Cout*(Cin+1)] */
    int nparts;               /* as returned by salt_head1x1_bwd_parts */
    float* gw;                /* [Cout][Cin] */
    float* gb;                /* [Cout] or NULL */
} salt_head1x1_bwd_args;
int salt_head1x1_bwd(const salt_head1x1_bwd_args*, void* stream);
int salt_head1x1_bwd_parts(const salt_head1x1_bwd_args*);
/* 1 head1x1_bwd_kernel (scalar), 2 head1x1_bwd_vec_kernel; < 0: refused (host only, no launch; tests) */
int salt_head1x1_bwd_kernel_id(const salt_head1x1_bwd_args*);

/* ------------------------------------------------------------------ BatchNorm2d (+ReLU, +residual)
 * torch semantics (eps 1e-5, momentum 0.1, biased batch variance for normalisation, unbiased for the
 * running estimate): unet_models.py:25,45,61; base.py:23; torchvision BasicBlock/Bottleneck. */
typedef struct {
    const float* stats;       /* [nparts][2][C] */
    const float* stats_cnt;   /* [nparts] */
    int nparts;
    int C;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    int64_t* num_batches_tracked;   /* may be NULL */
    float momentum;
    float eps;
    float* mean;              /* out [C] */
    float* invstd;            /* out [C] */
    float* scale;             /* out [C]: gamma*invstd */
    float* shift;             /* out [C]: beta - mean*scale */
} salt_bn_finalize_args;
int salt_bn_finalize(const salt_bn_finalize_args*, void* stream);
/* floats the `stats` workspace must hold for nparts partials of C channels (partials + chunk heads) */
int64_t salt_bn_stats_floats(int nparts, int C);

typedef struct {              /* eval mode: scale/shift from running statistics */
    int C;
    const float* gamma;
    const float* beta;
    const float* running_mean;
    const float* running_var;
    float eps;
    float* scale;
    float* shift;
} salt_bn_fold_args;
int salt_bn_fold(const salt_bn_fold_args*, void* stream);

typedef struct {              /* a = relu?( y*scale + shift (+ res) ) */
    int dtype;
    salt_view y;
    const float* scale;       /* NULL = identity */
    const float* shift;
    salt_view res;            /* res.p == NULL: none */
    int relu;
    salt_view a;
    /* Consumer-side BatchNorm finalize: fin_acc != NULL (the [8][2 C + 1] fp64 shards a salt_conv launch with fin_acc and NO
     * fin_ticket added its statistics to; fin = the const salt_bn_finalize_args* of the layer): scale / shift are ignored - every
     * workgroup derives them from the shards, workgroup 0 stores mean / invstd / scale / shift and updates the running statistics.
     * The shards are NOT cleared (salt_zero them before the producer's next launch). */
    const void* fin;
    const double* fin_acc;
} salt_affine_act_args;
int salt_affine_act(const salt_affine_act_args*, void* stream);

typedef struct {              /* backward of a = relu?(bn(y) (+res)) in train mode */
    int dtype;
    salt_view da;             /* grad wrt a */
    salt_view a;              /* forward output (ReLU mask).  a.p == NULL: relu == 0, or (no residual) recompute the mask from y */
    salt_view y;              /* conv output (pre-BN) */
    int relu;
    const float* mean;
    const float* invstd;
    const float* gamma;
    const float* beta;        /* needed when the mask is recomputed from y */
    float* partials;          /* [nparts][2][C] workspace */
    int nparts;               /* as returned by salt_bn_bwd_parts */
    float* dgamma;            /* [C] */
    float* dbeta;             /* [C] */
    int accumulate_param_grads;
    float* coef;              /* [3][C] workspace: k, c1, c2 */
    salt_view dy;             /* out: grad wrt y */
    salt_view dres;           /* out: grad wrt residual (masked da); dres.p == NULL: none */
    int accumulate_dres;
    int partials_ready;       /* 1: `partials` ([nparts][2][C], any nparts >= 1) was filled by the producer of da (salt_conv_args.bnb_*) */
                              /* 2: the producer also finalized (salt_conv_args.bnb_fin): coef / dgamma / dbeta are ready, only the apply pass runs */
                              /* 3: the producer added the sums to fin_acc (salt_conv_args.bnb_acc without ticket): the apply pass finalizes them */
    double* fin_acc;          /* partials_ready == 0 and fin_acc != NULL: the reduction pass accumulates into [8][2][C] fp64 shards and its last block */
    const float* da_bias;     /* NULL, or [B][C]: a per-image, per-channel constant added to da wherever it is read (partials_ready 0, or 3 when the sums in fin_acc already include it) */
    uint32_t* fin_ticket;     /* finalizes (no partials, no finalize launch); both zero before the first call, left zero (see salt_conv_args.fin).
                               * fin_ticket == NULL: no in-launch finalize - the apply pass finalizes the shards; the caller clears them */
    /* round 6 - secondary sums (apply pass with fin_acc and no ticket, dres written without accumulate_dres): the residual branch is the
     * output of ANOTHER train-mode BatchNorm without ReLU (a ResNet projection shortcut, torchvision layout through
     * architectures/encoders.py:38-45) whose dL/da is exactly the dres this call stores - the pass also takes that layer's
     * BatchNorm-backward sums (sum dres, sum dres xhat_sec with xhat_sec from sec_y / sec_mean / sec_invstd) into the fp64 shards
     * sec_acc [8][2][C] (zero on entry), so the shortcut's own salt_bn_bwd runs with partials_ready 3 and no reduction pass */
    salt_view sec_y;
    const float* sec_mean;
    const float* sec_invstd;
    double* sec_acc;
} salt_bn_bwd_args;
int salt_bn_bwd(const salt_bn_bwd_args*, void* stream);
int salt_bn_bwd_parts(const salt_bn_bwd_args*);

/* ------------------------------------------------------------------ train-mode BatchNorm + ReLU + 1x1 logit head in ONE pass (round 6)
 * The reference's `final` Sequential (architectures/unet.py:84-87: Conv2dBnRelu -> nn.Conv2d(C, num_classes, 1)) in TRAINING: the
 * activation a = relu(bn(y)) has exactly one reader, the 1x1 head, and the head's input gradient exactly one reader, the BatchNorm
 * backward - so neither tensor needs to exist.  salt_head_bn finalizes the statistics shards of y's producer (consumer side, like
 * salt_affine_act with fin_acc), applies scale / shift / ReLU to y on the way in, rounds to the storage dtype exactly where
 * salt_affine_act would have stored, and writes the fp32 NCHW logits.  salt_head_bn_bwd is the matching backward in two passes
 * over y: (1) head weight / bias gradients and the BatchNorm-backward sums of da = W^T dlogits (recomputed per pixel: rank
 * num_classes) into fp64 shards, (2) dy = k (mask da - c1 - xhat c2) with the sums finalized in every workgroup's prologue (like
 * salt_bn_bwd with partials_ready 3).  Replaces salt_affine_act + salt_head1x1 and salt_head1x1_bwd + salt_bn_bwd for that layer:
 * 0.47 GB of traffic -> 0.21 GB at the C2 shape. */
typedef struct {
    int dtype;
    salt_view y;              /* RAW convolution output (pre-BatchNorm) [B,H,W,C]; C / (16-byte piece) a power of two <= 64 */
    const void* fin;          /* const salt_bn_finalize_args* of the layer */
    const double* fin_acc;    /* [8][2 C + 1] fp64 statistics shards the producer of y added to (not cleared here) */
    int relu;
    const float* w;           /* head weight [Cout][C] fp32, Cout <= 4 */
    const float* bias;        /* [Cout] or NULL */
    int Cout;
    float* y_nchw;            /* out: fp32 logits [B,Cout,H,W] */
} salt_head_bn_args;
int salt_head_bn(const salt_head_bn_args*, void* stream);

typedef struct {
    int dtype;
    salt_view y;              /* raw convolution output, as in the forward call */
    int relu;
    const float* mean;        /* [C] batch statistics the forward call stored */
    const float* invstd;
    const float* gamma;
    const float* beta;
    const float* w;           /* head weight [Cout][C] */
    int Cout;
    const float* dy_nchw;     /* d loss / d logits, fp32 [B,Cout,H,W] */
    float* partials;          /* workspace [nparts][Cout (C + 1)] */
    int nparts;               /* as returned by salt_head_bn_bwd_parts */
    float* gw;                /* out: head weight gradient [Cout][C] */
    float* gb;                /* out: head bias gradient [Cout] or NULL */
    double* fin_acc;          /* [8][2][C] fp64 shards of the BatchNorm-backward sums, zero on entry (salt_zero), left filled */
    float* dgamma;            /* out [C] */
    float* dbeta;             /* out [C] */
    float* coef;              /* out [3][C] (k, c1, c2) or NULL */
    salt_view dy;             /* out: grad wrt y */
} salt_head_bn_bwd_args;
int salt_head_bn_bwd(const salt_head_bn_bwd_args*, void* stream);
int salt_head_bn_bwd_parts(const salt_head_bn_bwd_args*);

typedef struct {              /* backward of a = relu(y (+res)) without BN, or plain masked copy */
    int dtype;
    salt_view da;
    salt_view a;
    salt_view dy;
    int accumulate;
} salt_relu_bwd_args;
int salt_relu_bwd(const salt_relu_bwd_args*, void* stream);

/* ------------------------------------------------------------------ pooling / resize / layout */
typedef struct {              /* nn.MaxPool2d(2,2) (unet_models.py:119) */
    int dtype;
    salt_view x;
    salt_view y;
} salt_maxpool2_args;
int salt_maxpool2(const salt_maxpool2_args*, void* stream);

typedef struct {              /* gradient to the first maximal element of each window (torch rule) */
    int dtype;
    salt_view x;
    salt_view dy;
    salt_view dx;
    int accumulate;
} salt_maxpool2_bwd_args;
int salt_maxpool2_bwd(const salt_maxpool2_bwd_args*, void* stream);
/* nn.MaxPool2d(3, stride 2, padding 1): the ResNet stem pool of ResNetEncoders(pool0=True) (architectures/encoders.py:23-27); same
 * argument structs, y / dy are ceil(H/2) x ceil(W/2); the gradient goes to the first maximum of every (overlapping) window */
int salt_maxpool3s2(const salt_maxpool2_args*, void* stream);
int salt_maxpool3s2_bwd(const salt_maxpool2_bwd_args*, void* stream);

typedef struct {              /* nn.AvgPool2d(2,2) (unet.py:62); bwd: dx = dy/4 */
    int dtype;
    salt_view x;
    salt_view y;
    int backward;             /* 0: y = avg(x);  1: x(+)= y/4 broadcast (x is the grad output) */
    int accumulate;
} salt_avgpool2_args;
int salt_avgpool2(const salt_avgpool2_args*, void* stream);

typedef struct {              /* bilinear xR (nn.Upsample / F.upsample(mode='bilinear'), base.py:70, unet.py:103-106) */
    int dtype;
    salt_view x;              /* low resolution  [B,H,W,C] */
    salt_view y;              /* high resolution [B,H*R,W*R,C] */
    int R;
    int backward;             /* 0: y = up(x);  1: x (+)= up^T(y) */
    int accumulate;
    void* tmp;                /* backward, R >= 4: workspace of B*(H*R)*W*roundup(C) elements for the separable adjoint, or NULL */
    int align_corners;        /* 0: src = (dst + 0.5) / R - 0.5 clamped at 0 (torch >= 0.4 default: what the oracle / goldens executed);
                               * 1: src = dst * (H - 1) / (R H - 1) - how torch 0.3.1, the reference's pinned version (environment.yml:17),
                               * evaluated the same call: use it for checkpoints trained in the reference's own environment */
} salt_bilinear_args;
int salt_bilinear(const salt_bilinear_args*, void* stream);

/* Factored hypercolumn (architectures/unet.py:101-109 + architectures/base.py:21-37).  The reference builds
 *   hyper = cat([dec1, up2(dec2), up4(dec3), up8(dec4), up16(dec5)])  and runs  Conv2dBnRelu(5 C, C): replicate pad (top 2, right 2), 3x3.
 * A 1x1 contraction over channels commutes with bilinear up-sampling and with the tap shift, so for an up-sampled level k
 *   conv3x3(pad(up_R(x_k)))[o, Y, X] = sum_{t = (kh, kw)} up_R(z_k[t])[o, max(Y + kh - 2, 0), min(X + kw, W - 1)],   z_k[t] = W[:, level k, kh, kw] x_k
 * with z_k computed at LOW resolution by one 1x1 convolution (Cin -> 9 Cout; salt_conv + the tap-GEMM pack above).  This operator is the
 * remaining stencil: forward   y = y_in + sum_k sum_t shift_t(up_R[k](z[k][t]))   (+ train-mode BatchNorm statistics of y through
 * fin_acc, or the eval epilogue relu?(y scale + shift)); backward (backward = 1): z[k] (gradients, overwritten) = adjoint of that sum
 * applied to y (the gradient of the convolution output).  The up-sampled level, its 9-tap convolution (R^2 times the MACs of the 1x1
 * at low resolution) and its weight-gradient slab never exist.  z[k] is [B, H / R[k], W / R[k], 9 C], channel t C + o = tap t = 3 kh + kw.
 * Views 16-byte aligned, C and every pixel stride multiples of 8; backward: W <= 256. */
typedef struct {
    int dtype;
    int nlev;                 /* 1..4 */
    salt_view z[4];
    int R[4];                 /* H / z[k].H, powers of two in 4 .. 32 (a x2 level gains nothing: its z is 9/4 of the up-sampled plane) */
    salt_view y_in;           /* forward: [B,H,W,C] partial sum (the convolution over the full-resolution operands); p == NULL: zero */
    salt_view y;              /* forward: out [B,H,W,C] (may alias y_in);  backward: the gradient read */
    int backward;
    int align_corners;        /* as salt_bilinear_args.align_corners */
    const float* scale;       /* forward, eval: y = relu?(y scale[c] + shift[c]); NULL: none */
    const float* shift;
    int relu;
    double* fin_acc;          /* forward, train: [8][2 C + 1] fp64 shards (sum, sum of squares, count) of y, as salt_conv_args.fin_acc without a ticket */
    /* forward, eval: the logit head nn.Conv2d(C, head_cout, 1) (architectures/unet.py:84-87: final = Sequential(Conv2dBnRelu, Conv2d 1x1),
     * its only consumer) applied to the epilogue's values as they would be STORED (rounded to dtype) - salt_head1x1's arithmetic and
     * summation order, bit-identical to running it on y.  With head_y_nchw set, y.p may be NULL: y (2 x 2.1 GB of traffic at
     * [64,256,256,256]) is then never written or read.  C = 64, 128, 256 (bf16: also 512); head_cout 1..2. */
    const float* head_w;      /* [head_cout][C] fp32 or NULL */
    const float* head_b;      /* [head_cout] or NULL */
    float* head_y_nchw;       /* fp32 [B, head_cout, H, W] */
    int head_cout;
    float* head_ws;           /* C > 64: fp32 workspace of B (C / 64) head_cout H W elements (per-channel-block values, joined in salt_head1x1's tree order) */
} salt_hyper_stencil_args;
int salt_hyper_stencil(const salt_hyper_stencil_args*, void* stream);

typedef struct {              /* adjoint of replicate padding: fold an extended grad back (base.py:21-27) */
    int dtype;
    salt_view xp;             /* [B,H+top+bottom,W+left+right,C] */
    int top;
    int bottom;
    int left;
    int right;
    salt_view x;              /* [B,H,W,C] */
    int accumulate;
} salt_pad_fold_args;
int salt_pad_fold(const salt_pad_fold_args*, void* stream);

typedef struct {              /* second half of the fused fold: y edge pixels += the pad ring a fold-mode salt_conv left in `strip` */
    int dtype;
    const void* strip;
    int strip_cs;
    int top;
    int bottom;
    int left;
    int right;
    salt_view x;              /* [B,H,W,C]: the unpadded gradient the convolution wrote */
} salt_pad_fold_strip_args;
int salt_pad_fold_strip(const salt_pad_fold_strip_args*, void* stream);
/* pixels per image of the ring: (top+bottom)*(W+left+right) + H*(left+right) */
int64_t salt_fold_strip_pixels(int H, int W, int top, int bottom, int left, int right);

typedef struct {              /* y = a + b (or y += a when b.p == NULL); also plain copy/cast between views */
    int dtype;
    salt_view a;
    salt_view b;
    salt_view y;
    int accumulate;
} salt_add_args;
int salt_add(const salt_add_args*, void* stream);

typedef struct {              /* fp32 NCHW [B,C,H,W] <-> NHWC view (dtype) */
    int dtype;
    float* nchw;
    salt_view nhwc;
    int to_nhwc;              /* 1: nchw -> nhwc, 0: nhwc -> nchw */
} salt_layout_args;
int salt_layout(const salt_layout_args*, void* stream);

/* ------------------------------------------------------------------ squeeze-excitation (base.py:82-117)
 * out = relu( x*cSE(x) + x*sSE(x) ),  cSE = sigmoid(W2 relu(W1 gap(x)+b1)+b2),  sSE = sigmoid(w.x+b) */
typedef struct {
    int dtype;
    salt_view x;
    const float* w1;          /* [R][C] */
    const float* b1;          /* [R] */
    const float* w2;          /* [C][R] */
    const float* b2;          /* [C] */
    int R;
    const float* ws;          /* [C] (sSE 1x1 conv weight) */
    const float* bs;          /* [1] */
    float* gap_partials;      /* [B][nparts][C] workspace */
    int nparts;               /* as returned by salt_scse_parts */
    float* gap;               /* [B][C]  (saved for backward) */
    float* hidden;            /* [B][R]  (saved, post-ReLU) */
    float* gate_c;            /* [B][C]  (saved) */
    float* gate_s;            /* [B][H*W] (saved) */
    salt_view y;
    double* gap_acc;          /* NULL, or [B][C] fp64 ZEROED by the caller: the pooling pass adds its channel sums there (atomics) and the
                                 apply pass derives the gates of its image in its prologue - two launches instead of three; gap_partials unused */
    /* round 6 - x is the RAW output of a train-mode convolution whose BatchNorm + ReLU (base.Conv2dBnRelu, architectures/base.py:29-36)
     * this launch applies on the way in: in_fin = the layer's const salt_bn_finalize_args*, in_fin_acc = the [8][2 C + 1] fp64 shards
     * its producer added to (gap_acc path only).  The pooling pass finalizes the statistics (workgroup 0 stores mean / invstd / scale /
     * shift and the running statistics), both passes evaluate a = round(relu(y scale + shift)) per element - the activation tensor
     * and the salt_affine_act launch that would have written it do not exist.  salt_scse_bwd gets the same transform (in_scale ..). */
    const void* in_fin;
    const double* in_fin_acc;
    int in_relu;
} salt_scse_args;
int salt_scse(const salt_scse_args*, void* stream);
int salt_scse_parts(const salt_scse_args*);

typedef struct {
    int dtype;
    salt_view x;
    salt_view y;              /* forward output (ReLU mask) */
    salt_view dy;
    const float* w1;
    const float* w2;
    int R;
    const float* ws;
    const float* gap;
    const float* hidden;
    const float* gate_c;
    const float* gate_s;
    float* partials;          /* [B][nparts][2C+1] workspace */
    int nparts;
    float* g_w1;
    float* g_b1;
    float* g_w2;
    float* g_b2;
    float* g_ws;
    float* g_bs;
    float* dgap;              /* [B][C] workspace */
    salt_view dx;
    int accumulate;
    double* acc;              /* NULL, or [B][2C+1] fp64 ZEROED by the caller: the first pass adds its per-part sums there (atomics) and the
                                 FC backward reads them - no parts-reduction launch; partials unused */
    int skip_bcast;           /* 1: dx is left WITHOUT the channel-SE term dgap[b][c]; the consumer of dx adds it on the fly
                                 (salt_bn_bwd_args.da_bias = dgap) - one full pass over dx less */
    const float* in_scale;    /* != NULL: x is the raw convolution output of salt_scse_args.in_fin; the forward call stored scale / shift */
    const float* in_shift;
    int in_relu;
    /* bnb_acc != NULL (needs acc, in_scale, skip_bcast): dx is dL/da of the Conv-BN-ReLU layer that produced x (minus dgap, which that
     * layer's salt_bn_bwd adds through da_bias) - the first pass also takes that layer's BatchNorm-backward sums per image and the
     * FC backward writes (sum, sum xhat) INCLUDING the dgap term to shard 0 of bnb_acc ([8][2][C] fp64, zero on entry): the layer's
     * salt_bn_bwd then runs with partials_ready 3 + da_bias and no reduction pass.  acc must then hold [B][6 C + 1] doubles. */
    const float* bn_mean;
    const float* bn_invstd;
    double* bnb_acc;
    /* 1 (needs acc): salt_scse_bwd leaves the parameter gradients g_w1 .. g_bs to salt_scse_fc_grads (same arguments, any stream ordered
     * behind this call - the weight-gradient queue) and computes dgap (+ the bnb_acc sums, spread over the shards by image) with one
     * workgroup per image instead of one workgroup for the batch: the parameter gradients are nobody's input before the optimizer */
    int defer_param_grads;
} salt_scse_bwd_args;
int salt_scse_bwd(const salt_scse_bwd_args*, void* stream);
int salt_scse_fc_grads(const salt_scse_bwd_args*, void* stream);

/* ------------------------------------------------------------------ depth-conditioned channel gate (architectures/base.py:120-131,
 * models_with_depth.py:56-76): s[b][j] = sigmoid(w[j] D[b] + bias[j]) (nn.Linear(1, C) + Sigmoid), hyper * s[:, :, None, None].
 * A per-image, per-channel scale commutes with bilinear up-sampling, so every hypercolumn level is gated at its OWN resolution by
 * salt_channel_gate over channels [c0, c0 + C) of the gate; no full-resolution 5d-channel tensor is ever formed. */
typedef struct {
    const float* d;           /* [B][1] fp32 depth of every image */
    const float* w;           /* [C] (nn.Linear(1, C).weight is [C][1]) */
    const float* bias;        /* [C] */
    int B;
    int C;
    float* s;                 /* [B][C] gate: written by forward, read by backward */
    int backward;             /* 0: s from d, w, bias.  1: gw[j] = sum_b ds s (1 - s) D[b], gb[j] = sum_b ds s (1 - s), b ascending */
    const float* ds;          /* backward: [B][C] fp32 dL/ds (the fixed-order path of salt_channel_gate), or NULL */
    const double* ds_acc;     /* backward: [B][C] fp64 sums salt_channel_gate added to (atomics path), used when ds == NULL */
    float* gw;                /* backward out [C] */
    float* gb;                /* backward out [C] */
    int accumulate;           /* 1: gw / gb += */
} salt_depth_gate_args;
int salt_depth_gate(const salt_depth_gate_args*, void* stream);

typedef struct {
    int dtype;
    salt_view x;              /* forward input.  backward: the forward input, or with inplace = 1 the forward OUTPUT (the input is gone) */
    salt_view y;              /* forward: output, y = x s[b][c0 + c] (may be x itself).  backward: dL/dy */
    salt_view dx;             /* backward: dL/dx = dL/dy s (may be y itself) */
    const float* s;           /* [B][sC] */
    int sC;
    int c0;
    int backward;
    int accumulate;           /* backward: dx += */
    int inplace;              /* backward: x holds y = x s, s > 0: sum dy x = (sum dy y) / s */
    float* ds;                /* backward, fixed-order path: [B][sC] fp32, columns [c0, c0 + C) are WRITTEN from the partials (second launch) */
    float* partials;          /* backward, fixed-order path: [B][nparts][C] workspace */
    int nparts;               /* as returned by salt_channel_gate_parts */
    double* ds_acc;           /* backward, atomics path (ds == NULL): [B][sC] fp64 ZEROED by the caller; every (image, part) adds its sums */
} salt_channel_gate_args;
int salt_channel_gate(const salt_channel_gate_args*, void* stream);
int salt_channel_gate_parts(const salt_channel_gate_args*);

/* ------------------------------------------------------------------ losses
 * Lovasz hinge, per image, both channels flattened together, F.elu variant
 * (lovasz_losses.py:81-115,21-33; models.py:326-328).  One workgroup per image: LSD radix sort of
 * the hinge errors (stable; ties keep flat-index order), label scan, Jaccard gradient, dot. */
typedef struct {
    const float* logits;      /* fp32 NCHW [B,C,H,W] */
    const float* target;      /* fp32 NCHW [B,C,H,W] in {0,1} */
    int B;
    int P;                    /* elements per image = C*H*W */
    uint32_t* ws_keys;        /* [2][B][P] workspace */
    uint32_t* ws_vals;        /* [2][B][P] workspace */
    float* loss_per_image;    /* [B] */
    float* loss;              /* [1]: mean over images * loss_scale */
    float* dlogits;           /* fp32 NCHW or NULL (forward only) */
    float loss_scale;         /* loss weight (models.py:194) and 1/world for data parallel */
    uint32_t* ws_split;       /* NULL, or [rows * salt_lovasz_split_words(N)] words: rows of >= 4096 elements are then sorted by several
                                 workgroups each (segments of 2048 positions, 1 + 4 + 1 launches); same positions, ties and gradients */
    int flags;                /* SALT_LOVASZ_* below; 0 (a zeroed field): per image, no void label - the behaviour before the field existed */
    float ignore;             /* SALT_LOVASZ_HAS_IGNORE: the void value of `target` */
    uint32_t* ws_flat;        /* NULL, or [rows * salt_lovasz_flat_words(N)] words: rows above 131072 elements are then sorted by the
                                 long-row form (histograms in global memory); without it such a row runs in one workgroup */
} salt_lovasz_args;
int salt_lovasz_hinge(const salt_lovasz_args*, void* stream);
/* words per row of salt_lovasz_args.ws_split (0: the split form does not apply to this size) */
int64_t salt_lovasz_split_words(int P);
/* The options of lovasz_hinge(logits, labels, per_image, ignore) and lovasz_softmax(probas, labels, only_present, per_image, ignore)
 * (lovasz_losses.py:81-115,173-210), as bits of `flags`.  Rows x N below: the hinge sorts B rows of N = P elements, batch-flat 1 row
 * of N = B P; the softmax form B C rows of N = HW, batch-flat C rows of N = B HW.
 *   BATCH_FLAT    per_image=False: one row over the whole batch in the order of view(-1) - the hinge's B P floats as they lie in
 *                 memory; for class c of the softmax form pixel (b, i) has flat index b HW + i and lives at probas[(b C + c) HW + i].
 *                 The loss is that row's (the mean of the C rows'); only loss_per_image[0] (loss_per_row[0 .. C)) is written.
 *   HAS_IGNORE    an element whose target EQUALS `ignore` is void (tested before target > 0.5 makes a label): it is sorted behind
 *                 every valid element, counts neither in k, c_k nor G, adds 0 to the loss and gets a gradient of exactly 0; the valid
 *                 elements have the positions and g_k of the reference's compacted list.  A row without a valid element has loss 0
 *                 and still counts in the mean.  Softmax form: row (b, c) reads its own target plane, so the caller writes `ignore`
 *                 into EVERY plane of a void pixel.
 *   ONLY_PRESENT  softmax form only: a class row with no positive among its valid elements is skipped (gradient exactly 0).  Per
 *                 image the loss is the mean over the image's present classes (0 if none) and the result the mean over the B images,
 *                 dprobas of row (b, c) scale by loss_scale / (B present_b); batch-flat it is the mean over the classes present
 *                 anywhere in the batch.  Needs ws_present.
 * Each form uses the shortest sort that fits N: one workgroup below 4096, the split form (ws_split) up to 131072, the long-row form
 * (ws_flat) above; a missing workspace falls back to one workgroup.  All forms give bit-identical gradients.
 * SALT_E_BADARG from host code, nothing launched: an unknown flag bit, ONLY_PRESENT on the hinge or without ws_present, a NaN `ignore`
 * with HAS_IGNORE, a row longer than the payload encodes (N > 2^31 - 4096; N > 2^30 with HAS_IGNORE, ONLY_PRESENT or the softmax
 * form's BATCH_FLAT, whose payload carries the void bit). */
#define SALT_LOVASZ_BATCH_FLAT 1
#define SALT_LOVASZ_ONLY_PRESENT 2
#define SALT_LOVASZ_HAS_IGNORE 4
/* words per row of ws_flat for a row of N elements (0: the long-row form does not apply to this size) */
int64_t salt_lovasz_flat_words(int64_t N);

/* 0.2*mean_c dice(sigmoid) + 0.9*BCEWithLogits (models.py:315-340,361-388), sums over the whole batch */
typedef struct {
    const float* logits;
    const float* target;
    int B;
    int C;
    int HW;
    float dice_weight;
    float bce_weight;
    float* partials;          /* [nparts][4] workspace */
    int nparts;               /* as returned by salt_bce_dice_parts */
    float* sums;              /* [3C+1] workspace (kept for backward) */
    float* loss;              /* [1] */
    float* dlogits;           /* or NULL */
    float loss_scale;
} salt_bce_dice_args;
int salt_bce_dice(const salt_bce_dice_args*, void* stream);
int salt_bce_dice_parts(const salt_bce_dice_args*);

/* ------------------------------------------------------------------ softmax head (model_params['activation'] = 'softmax')
 * p = softmax over the C channels of every pixel of fp32 NCHW logits, the pixel's maximum subtracted first (logits of +-80 give
 * finite results).  One thread per pixel, coalesced along HW; y may alias x.  2 <= C <= 4; anything else, a NULL pointer or
 * B, HW < 1 is SALT_E_BADARG from host code, nothing is launched. */
typedef struct {
    const float* x;           /* logits [B,C,HW] */
    float* y;                 /* probabilities [B,C,HW] */
    int B;
    int C;
    int HW;
} salt_softmax_args;
int salt_softmax(const salt_softmax_args*, void* stream);

/* Softmax Jacobian: dz_j = p_j (dp_j - sum_c p_c dp_c) per pixel.  dz may alias dp.  Same refusals as salt_softmax. */
typedef struct {
    const float* p;           /* probabilities [B,C,HW] (salt_softmax's output) */
    const float* dp;          /* d loss / d p */
    float* dz;                /* d loss / d logits */
    int B;
    int C;
    int HW;
} salt_softmax_bwd_args;
int salt_softmax_bwd(const salt_softmax_bwd_args*, void* stream);

/* Lovasz-softmax, lovasz_softmax(probas, labels, only_present=False, per_image=True, ignore=None) of lovasz_losses.py:173-210: for
 * every image b and class c, e_i = |fg_i - p[b,c,i]| with fg_i = (target[b,c,i] > 0.5), sorted descending (stable: ties keep
 * ascending pixel index), g = lovasz_grad(fg_sorted), L[b,c] = sum_k e_k g_k (no elu);  loss = loss_scale * mean of the B*C rows;
 * dprobas[b,c,i] = (fg_i ? -1 : +1) g_rank(i) loss_scale / (B C), exactly 0 where e_i == 0.  A row (b,c) is a contiguous run of HW
 * floats: the sort, the scan and the fp32 sequence of g are salt_lovasz_hinge's kernels with the absolute-error policy over
 * B*C rows of HW elements (split form for HW >= 4096 when ws_split is given; gradients bit-identical to the unsplit form).
 * `probas` may be any values in [0,1]; they need not sum to 1.  2 <= C <= 4, B, HW >= 1, else SALT_E_BADARG without a launch. */
typedef struct {
    const float* probas;      /* fp32 [B,C,HW] */
    const float* target;      /* fp32 one-hot [B,C,HW] in {0,1} */
    int B;
    int C;
    int HW;
    uint32_t* ws_keys;        /* [2][B*C][HW] workspace */
    uint32_t* ws_vals;        /* [2][B*C][HW] workspace */
    float* loss_per_row;      /* [B*C] */
    float* loss;              /* [1] */
    float* dprobas;           /* fp32 [B,C,HW] or NULL (forward only) */
    float loss_scale;
    uint32_t* ws_split;       /* NULL, or [rows * salt_lovasz_split_words(N)] words */
    int flags;                /* SALT_LOVASZ_* (see salt_lovasz_args); 0: per image, all classes, no void label */
    float ignore;             /* SALT_LOVASZ_HAS_IGNORE: the void value, written by the caller into every target plane of a void pixel */
    uint32_t* ws_flat;        /* NULL, or [rows * salt_lovasz_flat_words(N)] words */
    uint32_t* ws_present;     /* SALT_LOVASZ_ONLY_PRESENT: [B*C] words, the positives of every row */
} salt_lovasz_softmax_args;
int salt_lovasz_softmax(const salt_lovasz_softmax_args*, void* stream);

/* Dice + cross entropy on softmax probabilities (the intent of mixed_dice_cross_entropy_loss, models.py:343-388), target one-hot
 * WITH the background channel 0, y = argmax_c target (first maximum), N = B*HW, sums over the whole batch:
 *   CE = -(1/N) sum log p[b,y,i] (as logsumexp - z_y);  for c = 1 .. C-1: I_c = sum p_c t_c, D_c = sum p_c + sum t_c + smooth + 1e-7,
 *   dice_c = 1 - (2 I_c + smooth) / D_c;  loss = loss_scale (dice_weight mean_c dice_c + cross_entropy_weight CE).
 * The reference function's channel arithmetic (target[:, class_nr] against output channel class_nr + 1) assumes a target without a
 * background channel and is not reproduced.  A partial-sums pass (salt_bce_dice's parts-per-plane rule, one part = one image x one
 * run of pixels), a fixed-order finalize in double, and a gradient pass through the softmax Jacobian (skipped when dlogits is
 * NULL).  No floating-point atomics: reruns are bit-identical.  2 <= C <= 4, B, HW >= 1, else SALT_E_BADARG without a launch. */
typedef struct {
    const float* logits;      /* fp32 [B,C,HW] */
    const float* target;      /* fp32 one-hot [B,C,HW] */
    int B;
    int C;
    int HW;
    float dice_weight;        /* reference default 0.5 */
    float cross_entropy_weight; /* reference default 0.5 */
    float smooth;             /* reference default 0 */
    float* partials;          /* [nparts][3C+1] workspace: per class I, sum p, sum t; then the CE sum */
    int nparts;               /* as returned by salt_dice_ce_parts */
    float* sums;              /* [3C+1] workspace (kept for backward) */
    float* loss;              /* [1] */
    float* dlogits;           /* or NULL */
    float loss_scale;
} salt_dice_ce_args;
int salt_dice_ce(const salt_dice_ce_args*, void* stream);
int salt_dice_ce_parts(const salt_dice_ce_args*);

/* ------------------------------------------------------------------ optimizer (models.py:74-75,289-297)
 * torch.optim.Adam with L2-in-gradient weight decay over one flat fp32 parameter buffer. */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    const float* hyper;       /* device [8]: lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale */
} salt_adam_args;
int salt_adam(const salt_adam_args*, void* stream);

/* Adam + L2 AND the bf16 forward weight packs in one pass (round 5).  The forward packs of the 3x3 / 1x1 layers (97 % of a ResNet's
 * parameters) are re-derived from the fp32 masters after every optimizer step (salt_pack_batched: 405 MB of traffic, the first launch of
 * the next step on the critical queue).  Here the thread that updates 8 input channels x all taps of one output channel - 8 KK contiguous
 * floats of the master - also stores their KK 16-byte packed pieces: the same values salt_pack_batched would write, bit for bit.
 * `jobs` are the salt_pack_conv_weight_args of those layers (salt_pack_job_is_vec(job) != 0, each weight at most once, every `w` inside
 * [param, param + n)); `rest` lists the ranges of the flat buffer no job covers (everything else takes the plain update of salt_adam). */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    const float* hyper;       /* as salt_adam_args.hyper */
    const void* jobs;         /* DEVICE array of salt_pack_conv_weight_args */
    const int* job_block0;    /* DEVICE [njobs + 1]: prefix of salt_pack_job_blocks */
    int njobs;
    int pack_blocks;
    const int64_t* rest;      /* DEVICE [nrest][2]: (first element, element count), both multiples of 4 */
    const int* rest_block0;   /* DEVICE [nrest + 1]: prefix of ceil(count / 1024) */
    int nrest;
    int rest_blocks;
} salt_adam_pack_args;
int salt_adam_pack(const salt_adam_pack_args*, void* stream);
/* != 0 for the jobs salt_adam_pack can write on the way: salt_pack_batched's vector path, 3x3 layers (KH KW = 9) */
int salt_pack_job_is_vec(const salt_pack_conv_weight_args*);

typedef struct {              /* advance step counter and bias corrections on device (graph-replay safe) */
    float* hyper;             /* as above */
    int64_t* step;            /* device [1] */
} salt_adam_tick_args;
int salt_adam_tick(const salt_adam_tick_args*, void* stream);

typedef struct {
    void* p;
    int64_t bytes;
} salt_zero_args;
int salt_zero(const salt_zero_args*, void* stream);

/* ------------------------------------------------------------------ inference epilogue
 * sigmoid -> inverse flip (TTA) -> mean over variants (models.py:143-144, augmentation.py:156-163,
 * loaders.py:722-760);  flips are index permutations. */
typedef struct {
    const float* logits;      /* fp32 NCHW [V*B, C, H, W]: variant-major */
    int V;
    int B;
    int C;
    int H;
    int W;
    const int* flip_ud;       /* host arrays [V] */
    const int* flip_lr;
    float* prob;              /* fp32 NCHW [B,C,H,W] */
    const int* rot;           /* host array [V] or NULL: quarter turns k of the variant's forward np.rot90 (augmentation.py:143-153; H == W);
                               * the inverse applied here is rot90(-k), then fliplr, then flipud (augmentation.py:156-163) */
    int method;               /* aggregation over the variants (loaders.py:727-735): 0 mean, 1 max, 2 min, 3 gmean = exp(mean(log p)) */
    int activation;           /* 0 (a zeroed struct): sigmoid of `logits`; 1: none, `logits` holds probabilities already (the softmax
                               * head: salt_softmax over the [V*B,C,HW] logits first) */
} salt_tta_mean_args;
int salt_tta_mean(const salt_tta_mean_args*, void* stream);

typedef struct {              /* x_out[b] = flip(x[b]) for NCHW fp32 batches (TTA forward transform) */
    const float* x;
    int B;
    int C;
    int H;
    int W;
    int flip_ud;
    int flip_lr;
    float* y;
} salt_flip_args;
int salt_flip(const salt_flip_args*, void* stream);

/* ------------------------------------------------------------------ on-device input pipeline
 * gray tile -> [resize: cubic | bilinear] -> edge pad -> Normalize -> AddDepthChannels; mask -> [resize] -> pad -> one-hot
 * (loaders.py:603-612,763-769; augmentation.py:79-96,247-284; utils.py:494-500).  Normalisation divides by std exactly as
 * torchvision ((g - mean) / std is evaluated as (g - mean) * (1 / std), agreement 1 ulp). */
typedef struct {
    const void* img;          /* [B,h,w] uint8 (img_is_u8) or fp32 in [0,1] */
    int img_is_u8;
    const uint8_t* mask;      /* [B,h,w] {0,1} or NULL */
    int B;
    int h;
    int w;
    int resize_h;             /* 0 = no resize */
    int resize_w;
    int top;                  /* rows / columns of edge padding before the tile; the rest of [H,W] is padded after it */
    int left;
    int H;
    int W;
    int channels;             /* 1 (gray only) | 3 (gray, depth ramp, gray*ramp) */
    float mean[3];
    float std[3];
    float* x;                 /* out fp32 NCHW [B,channels,H,W] */
    float* target;            /* out fp32 NCHW [B,2,H,W] one-hot {background, salt}; required when mask != NULL */
    int interpolation;        /* of the resize.  1: cubic - cv2.INTER_CUBIC as imgaug 0.2.5's iaa.Scale default (augmentation.py:79-85 passes no
                               * interpolation; environment.yml:15-16): Keys kernel a = -0.75, half-pixel centres, replicated border; a uint8
                               * tile is rounded back to the uint8 grid with saturation (cv2's uint8 output) and the {0,1} mask goes through the
                               * same resize, then round-half-up (the FLOAT form of the filter).  2 (uint8 tiles only): the same filter as
                               * opencv_python 3.4.0.12 evaluates it on CV_8U - per-axis coefficients rounded to 11-bit fixed point
                               * (cvRound(c * 2048), each on its own), integer horizontal / vertical sums, saturate((v + 2^21) >> 22);
                               * differs from 1 by one LSB on a few percent of the pixels.  0: bilinear, half-pixel centres, nearest for
                               * the mask (rounds 1 - 2 default) */
    int pad_mode;             /* 0: edge (replicate: padded index clamped to the tile), 1: reflect-101 (cv2.BORDER_REFLECT_101 of PadFixed,
                               * augmentation.py:99-101 = np.pad(mode='reflect') of imgaug 0.2.5's Pad at inference): index i of an axis of n
                               * -> -i for i < 0, 2 n - 2 - i for i >= n; needs pad <= n - 1 on every side (else SALT_E_BADARG).  Applied
                               * where the clamp is: on the resized grid, image and mask alike; everything after the pad is unchanged */
} salt_preprocess_args;
int salt_preprocess(const salt_preprocess_args*, void* stream);

/* on-device training augmentation fused with the train-branch preprocessing (main.py:130-133, loaders.py:124-150,
 * augmentation.py:34-65).  Per image b (one workgroup, planes in LDS, every stage written back onto the uint8 grid with
 * round-half-up + clip; the mask is binarised (!= 0) after every stage):
 *   affine_seq: stages A | B | C in a random permutation
 *     A  SomeOf((1, 2), [Fliplr(p), Sharpen(alpha, lightness), Emboss(alpha, strength), Affine(rotate, translate x, mode edge)]),
 *        picks among the ENABLED children only, applied in list order (no child enabled: A is a no-op)
 *     B  Sometimes(p, PiecewiseAffine(scale)): 4x4 control points at linspace(0, h, 4) x linspace(0, w, 4) jittered by
 *        N(0, s) * h (y) / N(0, s) * w (x); every grid cell is split along its top-left -> bottom-right diagonal; the output pixel's
 *        triangle of the regular grid maps affinely onto the jittered triangle; bilinear, 0 outside
 *     C  Sometimes(p, PerspectiveTransform(scale)): corners tl (jx, jy), tr (w - jx, jy), br (w - jx, h - jy), bl (jx, h - jy) with
 *        j = (|N(0, s)| mod 1) * size; rectified size max(int(|br - bl|), int(|tr - tl|)) x max(int(|bl - tl|), int(|br - tr|)),
 *        clamped to [2, SALT_AUG_RECT_MAX]; bilinear, 0 outside; then the float cubic (a = -0.75, replicated border) back to h x w
 *   resize + edge pad exactly as salt_preprocess interpolation 2 (the fixed-point cubic)
 *   intensity_seq on the padded uint8 grid: Invert(p), Sometimes(p, ContrastNormalization(alpha)), OneOf([Noop, OneOf([Add,
 *     AddElementwise, Multiply, MultiplyElementwise])]) (Noop with p_noop, else uniform among the enabled four)
 *   Normalize + AddDepthChannels + one-hot target exactly as salt_preprocess.
 * RNG (splitmix64; all arithmetic mod 2^64):
 *   mix(z) = z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 *   key    = mix(mix(mix(seed) ^ counter) ^ b);   bits(slot) = mix(key + slot * 0x9E3779B97F4A7C15)
 *   uniform u = (bits >> 40) * 2^-24 (float, exact);  integer in [lo, hi]: lo + ((bits >> 32) * (hi - lo + 1) >> 32)
 *   float in [lo, hi): lo + u * (hi - lo) (float32, rounded per operation);  normal k: Box-Muller on slots 64 + 2k, 65 + 2k with
 *   u1 = ((bits >> 40) + 1) * 2^-24, sqrt(-2 ln u1) * cos(2 pi u2)
 *   per-pixel draws (AddElementwise / MultiplyElementwise) use slot 1024 + Y * W + X of the padded output grid.
 * Parameter slots: 0 order, 1 SomeOf n, 2 / 3 SomeOf picks, 4 flip, 5 angle, 6 shift, 7 / 8 piecewise on / scale, 10 / 11 perspective
 *   on / scale, 12 invert, 13 / 14 contrast on / alpha, 15 / 16 intensity Noop / pick, 17 add / multiply value.
 * Enable bits and probabilities apply to drawing; a replayed record (params_given) is applied as it is. */
#define SALT_AUG_FLIPLR 1
#define SALT_AUG_SHARPEN 2
#define SALT_AUG_EMBOSS 4
#define SALT_AUG_AFFINE 8
#define SALT_AUG_PIECEWISE 16
#define SALT_AUG_PERSPECTIVE 32
#define SALT_AUG_INVERT 64
#define SALT_AUG_CONTRAST 128
#define SALT_AUG_ADD 256
#define SALT_AUG_ADD_ELEMENTWISE 512
#define SALT_AUG_MULTIPLY 1024
#define SALT_AUG_MULTIPLY_ELEMENTWISE 2048
#define SALT_AUG_MAX_TILE 128     /* h, w <= this */
#define SALT_AUG_RECT_MAX 182     /* rectified perspective edge <= ceil(tile diagonal) */
/* params record, fp32 [B, SALT_AUG_PARAMS] per image:
 *   0 stage order: index into the permutations of (A, B, C) in lexicographic order: ABC ACB BAC BCA CAB CBA
 *   1 SomeOf n (0: A applies nothing)         2..5 chosen: Fliplr, Sharpen, Emboss, Affine (0 / 1)
 *   6 flip fires (0 / 1)                      7 rotation, degrees            8 shift, fraction of w (pixels = shift * w)
 *   9 piecewise on (0 / 1)                    10 piecewise scale             11..42 jitter of control point k = 4 i + j: (dy, dx)
 *                                                                                    at 11 + 2k, 12 + 2k, fractions of h / w
 *   43 perspective on (0 / 1)                 44 perspective scale           45..52 corner offsets (x, y) of tl, tr, br, bl,
 *                                                                                    fractions of w / h in [0, 1)
 *   53 invert (0 / 1)                         54 contrast on (0 / 1)         55 contrast alpha
 *   56 intensity op: 0 Noop, 1 Add, 2 AddElementwise, 3 Multiply, 4 MultiplyElementwise
 *   57 Add value (integer) or Multiply factor  58..63 zero */
#define SALT_AUG_PARAMS 64
typedef struct {
    int enable;               /* SALT_AUG_* bits */
    float p_fliplr;           /* 0.5 */
    float sharpen_alpha;      /* 0.5; matrix (1 - alpha) I + alpha [[-1,-1,-1],[-1,8+L,-1],[-1,-1,-1]] */
    float sharpen_lightness;  /* 1 */
    float emboss_alpha;       /* 0.5; matrix (1 - alpha) I + alpha [[-1-s,-s,0],[-s,1,s],[0,s,1+s]] */
    float emboss_strength;    /* 1 */
    float rotate_min;         /* -10 degrees */
    float rotate_max;         /* 10 */
    float shift_min;          /* -0.05 of w */
    float shift_max;          /* 0.05 */
    float p_piecewise;        /* 0.3 */
    float piecewise_scale_min;  /* 0.04 */
    float piecewise_scale_max;  /* 0.08 */
    float p_perspective;      /* 0.3 */
    float perspective_scale_min;  /* 0.05 */
    float perspective_scale_max;  /* 0.1 */
    float p_invert;           /* 0.3 */
    float p_contrast;         /* 0.3 */
    float contrast_min;       /* 0.5 */
    float contrast_max;       /* 1.5 */
    float p_intensity_noop;   /* 0.5 */
    int add_min;              /* -10 (Add and AddElementwise, discrete uniform) */
    int add_max;              /* 10 */
    float mul_min;            /* 0.95 (Multiply and MultiplyElementwise) */
    float mul_max;            /* 1.05 */
} salt_augment_config;
typedef struct {
    const uint8_t* img;       /* [B,h,w] uint8, h, w <= SALT_AUG_MAX_TILE */
    const uint8_t* mask;      /* [B,h,w] {0,1} (binarised != 0) or NULL */
    int B;
    int h;
    int w;
    int resize_h;             /* 0 = no resize; otherwise the fixed-point cubic of salt_preprocess interpolation 2 */
    int resize_w;
    int top;
    int left;
    int H;
    int W;
    int channels;             /* 1 | 3 */
    float mean[3];
    float std[3];
    float* x;                 /* out fp32 NCHW [B,channels,H,W] */
    float* target;            /* out fp32 NCHW [B,2,H,W]; required when mask != NULL */
    salt_augment_config cfg;
    uint64_t seed;
    uint64_t counter;         /* the draws of image b are a pure function of (seed, counter, b) */
    float* params;            /* [B, SALT_AUG_PARAMS] record: written when drawing, read when params_given; NULL = not recorded */
    int params_given;         /* 1: replay `params` instead of drawing (per-pixel noise still from (seed, counter, b, pixel)) */
    uint8_t* geo_img;         /* debug out [B,h,w]: the tile after the geometric stages, or NULL */
    uint8_t* geo_mask;        /* debug out [B,h,w]: the binarised mask after the geometric stages, or NULL */
    uint8_t* gray;            /* debug out [B,H,W]: the padded tile after the intensity stage, or NULL */
    int pad_mode;             /* 0 edge | 1 reflect-101, as salt_preprocess_args.pad_mode */
} salt_augment_preprocess_args;
int salt_augment_preprocess(const salt_augment_preprocess_args*, void* stream);

/* centre crop + binarize one class of a probability map (postprocessing.py:24-43, utils.py:308-313): mask = prob[cls] > threshold */
typedef struct {
    const float* prob;        /* fp32 NCHW [B,C,H,W] */
    int B;
    int C;
    int H;
    int W;
    int cls;
    int top;                  /* crop window [top, top+h) x [left, left+w) */
    int left;
    int h;
    int w;
    float threshold;
    uint8_t* mask;            /* out [B,h,w] in {0,1} */
} salt_crop_threshold_args;
int salt_crop_threshold(const salt_crop_threshold_args*, void* stream);

/* validation metric counts for a whole threshold sweep in one pass (callbacks.py:503-513, metrics.py:21-66): per image and
 * threshold t: |pred_t| and |pred_t & gt| with pred_t = (double)prob[cls] > t on the cropped window; plus |gt| per image.
 * IoU / IOUT (with the reference's empty-mask conventions) follow on the host from these integers. */
#define SALT_MAX_THRESHOLDS 32
typedef struct {
    const float* prob;        /* fp32 NCHW [B,C,H,W] */
    int B;
    int C;
    int H;
    int W;
    int cls;
    int top;
    int left;
    int h;
    int w;
    const uint8_t* gt;        /* [B,h,w] in {0,1} */
    int T;
    const double* thresholds; /* HOST array [T], T <= SALT_MAX_THRESHOLDS */
    int* inter;               /* out [B][T] */
    int* pred;                /* out [B][T] */
    int* gt_count;            /* out [B] */
} salt_iou_sweep_args;
int salt_iou_sweep(const salt_iou_sweep_args*, void* stream);

/* ------------------------------------------------------------------ loader modes 'resize' / 'stacking' (csrc/resize.hip)
 * The reference's second-level data path (loaders.py:564-579, 786-795; postprocessing.py:8-21) and its `loader_mode: resize`.
 * skimage / imgaug / cv2 are not executable where this library is built, so every formula below is RESTATED from their sources
 * (skimage 0.14, PIL) and pinned against scipy.ndimage / PIL by the CPU tests; DESIGN.md 23 has the provenance.
 *
 * Source coordinates, all in float64, every operation rounded on its own (no fused multiply-add):
 *     s_r = h_in / h_out,  r(i) = s_r * (i + 0.5) - 0.5;   s_c = w_in / w_out,  c(j) = s_c * (j + 0.5) - 0.5
 * BILINEAR64(P, r, c), P a [h_in, w_in] map that reads 0 outside [0, h_in) x [0, w_in):
 *     r0 = floor(r), dr = r - r0, c0 = floor(c), dc = c - c0
 *     top = (1 - dc) * P(r0, c0)     + dc * P(r0, c0 + 1)
 *     bot = (1 - dc) * P(r0 + 1, c0) + dc * P(r0 + 1, c0 + 1)
 *     v   = (1 - dr) * top + dr * bot                                  (float64; fp32 taps are widened exactly)
 *
 * salt_stack_resize: ResizeArray + to_tensor_stacking in one launch (skimage.transform.resize(order 1, mode 'constant', cval 0, no
 * anti-aliasing) of every map: the border output pixels of an up-scale are blended with the zero outside, as the reference's are).
 *     y[b, m, i, j] = (float)BILINEAR64(x[b, :, :, m], r(i), c(j))     one rounding, to fp32
 * The input is addressed by element strides, so both layouts a caller holds are one entry point:
 *     [B,h,w,M] (np.stack(maps, axis=-1) per tile, utils.py:580): sb = h w M, sr = w M, sc = M, sm = 1
 *     [B,M,h,w] (per-model planes):                                 sb = M h w, sr = w, sc = 1, sm = h w
 * 1 <= M <= SALT_STACK_RESIZE_MAX_MAPS; h, w, H, W <= SALT_RESIZE_MAX_SIDE; B <= 65535 (one grid plane per image). */
#define SALT_STACK_RESIZE_MAX_MAPS 64
#define SALT_RESIZE_MAX_SIDE 256
typedef struct {
    const float* x;           /* fp32 maps, element (b, r, c, m) at x[b sb + r sr + c sc + m sm] */
    int B;
    int h;
    int w;
    int M;
    int64_t sb;               /* element strides, all > 0; sm == 1 or sc == 1 */
    int64_t sr;
    int64_t sc;
    int64_t sm;
    int H;
    int W;
    float* y;                 /* out fp32 NCHW [B,M,H,W], contiguous */
} salt_stack_resize_args;
int salt_stack_resize(const salt_stack_resize_args*, void* stream);

/* salt_mask_resize: the stacking target (loaders.py:355-360, 572-575).  For class k in (0, 1): Image.fromarray((mask == k) as uint8)
 * -> transforms.Resize((H, W)) = PIL BILINEAR -> convert('L') -> float32; the two classes are resized independently.
 * PIL's 8-bit resample is TWO passes, horizontal then vertical, the intermediate rounded onto the uint8 grid:
 *     per axis (n_in -> n_out): scale = n_in / n_out, support = max(scale, 1), centre(x) = (x + 0.5) scale
 *     window [start, start + len) = [max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in))
 *     weight of tap t: triangle((t - centre + 0.5) * (1 / support)), triangle(u) = max(1 - |u|, 0), times 1 / (their sum) (float64)
 *     t[r, j]      = floor(sum_t wc[j][t] * (mask[b, r, cstart[j] + t] == k) + 0.5)          horizontal, all float64
 *     target[b, k, i, j] = floor(sum_t wr[i][t] * t[rstart[i] + t, j] + 0.5)                 vertical
 * The tables are built by the caller in float64 and passed in (DEVICE arrays); the kernel rounds nothing but the two floor(x + 0.5).
 * The horizontal intermediate lives in registers and is never stored. */
typedef struct {
    const uint8_t* mask;      /* [B,h,w] */
    int B;
    int h;
    int w;
    int H;
    int W;
    const int* row_start;     /* DEVICE [H]: first source row of output row i */
    const int* row_len;       /* DEVICE [H]: 1 <= len <= row_taps, row_start + row_len <= h */
    const double* row_w;      /* DEVICE [H][row_taps] */
    int row_taps;
    const int* col_start;     /* DEVICE [W] */
    const int* col_len;       /* DEVICE [W] */
    const double* col_w;      /* DEVICE [W][col_taps] */
    int col_taps;
    float* target;            /* out fp32 NCHW [B,2,H,W] */
} salt_mask_resize_args;
int salt_mask_resize(const salt_mask_resize_args*, void* stream);

/* postprocessing.resize_image on a (C,H,W) probability array with a (C,h,w) target (skimage 0.14's n-D branch:
 * scipy.ndimage.map_coordinates(order 1, mode 'constant') at (channel, r(i), c(j)), no anti-aliasing): BILINEAR64 per channel.
 * h <= H and w <= W only (every coordinate then lies inside the source; an up-scale through this path is refused).
 * salt_resize_prob stores (float)v.  salt_resize_threshold and salt_resize_iou_sweep decide on the float64 interpolant v itself
 * (the reference thresholds the float64 array, postprocessing.py:41-43), which is never stored. */
typedef struct {
    const float* prob;        /* fp32 NCHW [B,C,H,W] */
    int B;
    int C;
    int H;
    int W;
    int h;
    int w;
    float* out;               /* out fp32 NCHW [B,C,h,w] */
} salt_resize_prob_args;
int salt_resize_prob(const salt_resize_prob_args*, void* stream);

typedef struct {
    const float* prob;        /* fp32 NCHW [B,C,H,W] */
    int B;
    int C;
    int H;
    int W;
    int cls;
    int h;
    int w;
    double threshold;
    uint8_t* mask;            /* out [B,h,w] in {0,1}: v > threshold */
} salt_resize_threshold_args;
int salt_resize_threshold(const salt_resize_threshold_args*, void* stream);

/* the counts of salt_iou_sweep with pred_t = v > t on the resized interpolant, against original-size masks */
typedef struct {
    const float* prob;        /* fp32 NCHW [B,C,H,W] */
    int B;
    int C;
    int H;
    int W;
    int cls;
    int h;
    int w;
    const uint8_t* gt;        /* [B,h,w] in {0,1} */
    int T;
    const double* thresholds; /* HOST array [T], T <= SALT_MAX_THRESHOLDS */
    int* inter;               /* out [B][T] */
    int* pred;                /* out [B][T] */
    int* gt_count;            /* out [B] */
} salt_resize_iou_sweep_args;
int salt_resize_iou_sweep(const salt_resize_iou_sweep_args*, void* stream);

/* ------------------------------------------------------------------ ensembling between models (csrc/ensemble.hip)
 * What the reference does with the predictions of several trained networks: main.py:892-912 (save_predictions: the mean over the
 * cross-validation folds, binarized and run-length encoded), notebooks/prediction_average.ipynb (the same across experiments, in a
 * float64 accumulator), utils.py:560-581 (channel 1 of every first-level model stacked with np.stack(axis=-1) for the second level).
 *
 * salt_ensemble: ONE pass over K member maps p_k, fp32 NCHW [B,C,H,W] each, up to three outputs.
 *   the member's value at output pixel (y, x) of channel c:
 *     mode 0 (postprocessing.crop_image):  v_k = p_k[b, c, top + y, left + x]                                   (the fp32 itself)
 *     mode 1 (postprocessing.resize_image): v_k = BILINEAR64(p_k[b, c], r(y), c(x)), H x W -> h x w             (float64, never stored;
 *                                           the same source text as salt_resize_prob: resize-each-then-mean, h <= H and w <= W)
 *   the mean, members added in ASCENDING k, the accumulator starting at member 0 (np.mean(np.array(maps), axis=0)):
 *     acc 0: s = v_0; s = fl32(s + v_k) for k = 1 .. K-1; mean = fl32(s / (float)K), one correctly rounded division;
 *            mask = mean[cls] > (float)threshold
 *     acc 1: the same in float64: s = (double)v_0; s = s + v_k; v = s / (double)K; mean = (float)v; mask = v[cls] > threshold,
 *            decided on the float64 value as salt_resize_threshold decides
 *   mode 1 with acc 0 is SALT_E_UNSUPPORTED (the reference's resized maps are float64).
 *   the stack, no averaging: stack[b sb + y sr + x sc + (m0 + k) sm] = (float)v_k of channel cls
 *     [B,h,w,M] (np.stack(maps, axis=-1), utils.py:580):              sb = h w M, sr = w M, sc = M, sm = 1
 *     [B,M,h,w] (StackingPreprocessor(layout='mhw')):                 sb = M h w, sr = w,   sc = 1, sm = h w
 *   with M >= m0 + K: a caller fills a slice of a wider stack, the other slots are not touched.
 * Refused without a launch (SALT_E_BADARG): NULL args, K outside 1 .. SALT_MAX_MEMBERS, a NULL member, a window outside the map,
 * an up-scale, cls outside [0, C), no output requested, a stack without positive strides. */
#define SALT_MAX_MEMBERS 64
typedef struct {
    const float* const* members;  /* HOST array [K] of device pointers, each fp32 NCHW [B,C,H,W]; 1 <= K <= SALT_MAX_MEMBERS */
    int K;
    int B;
    int C;
    int H;
    int W;
    int mode;                 /* 0: crop window [top,top+h) x [left,left+w); 1: resize H x W -> h x w */
    int top;
    int left;
    int h;
    int w;
    int acc;                  /* 0: fp32 accumulator, 1: float64 accumulator */
    float* mean;              /* out fp32 [B,C,h,w] or NULL */
    int cls;
    double threshold;
    uint8_t* mask;            /* out [B,h,w] in {0,1} or NULL */
    float* stack;             /* out or NULL: member k's class-`cls` map at stack[b*sb + y*sr + x*sc + (m0+k)*sm] */
    int64_t sb;
    int64_t sr;
    int64_t sc;
    int64_t sm;
    int m0;
} salt_ensemble_args;
int salt_ensemble(const salt_ensemble_args*, void* stream);

/* salt_rle_encode: utils.run_length_encoding (utils.py:99-111) of a batch of masks.  Pixel p = x h + y (COLUMN-major, x.T.flatten());
 * a run is a maximal range [s, e] of set positions (it continues from the bottom of a column into the top of the next); image b's
 * runs, in ascending s, are the pairs (s + 1, e - s + 1).  counts[b] is their number; the pairs of all images are packed: image b's
 * begin at pair index sum(counts[0 .. b)).  Two launches (count, then place at the exclusive prefix of counts), one 256-thread
 * workgroup per image, no atomics: the output is deterministic. */
typedef struct {
    const uint8_t* mask;      /* [B,h,w], nonzero = set; 1 <= h*w <= 65536 */
    int B;
    int h;
    int w;
    int* counts;              /* out [B]: runs of image b */
    int* runs;                /* out, packed pairs (start, length), start 1-based */
    int64_t cap_pairs;        /* pairs `runs` holds; a pair whose packed index is >= cap_pairs is NOT written */
    int64_t* total;           /* out [1]: sum(counts), also when it exceeds cap_pairs */
} salt_rle_encode_args;
int salt_rle_encode(const salt_rle_encode_args*, void* stream);

/* ------------------------------------------------------------------ program executor
 * A training/inference step is a static list of the operators above.  The host builds it once per
 * (model, batch shape); running it is one call.  capture/replay wraps it in a hipGraph. */
typedef int (*salt_op_fn)(const void* args, void* stream);
typedef struct {
    salt_op_fn fn;
    const void* args;
    int stream;               /* 0 = main, 1 = side, 2 = main after joining side work of this range, 3 = main after joining the side
                                 stream unconditionally (work enqueued there before the call) - salt_program_run_streams */
    int reserved;
} salt_program_entry;
int salt_program_run(const salt_program_entry* entries, int n, void* stream);
int salt_program_run_range(const salt_program_entry* entries, int begin, int end, void* stream);
/* as run_range, with a HIP event pair around every entry on `stream`; ms_out[i] = elapsed ms of entry begin+i */
int salt_program_run_timed(const salt_program_entry* entries, int begin, int end, void* stream, float* ms_out);
/* Two-stream execution: entries with stream == 1 (weight-gradient kernels) are enqueued on `side`, ordered after every
 * main-stream entry that precedes them in the list (event record/wait), and `main` re-joins `side` at the end of the range.
 * A main-stream entry that depends on side entries inside the range is tagged stream == 2: main waits for the side stream
 * right before it (forward: independent branches such as the hypercolumn up-samplings; backward: nothing - side entries only
 * produce parameter gradients).  side == NULL or side == main degenerates to salt_program_run_range. */
int salt_program_run_streams(const salt_program_entry* entries, int begin, int end, void* main_stream, void* side_stream);
/* join_at_end == 0: the caller orders its consumers after BOTH streams itself (bucketed all-reduce between backward segments) */
int salt_program_run_streams_ex(const salt_program_entry* entries, int begin, int end, void* main_stream, void* side_stream, int join_at_end);
/* ... with MARKS: before entry marks[m] (ascending, begin <= marks[m] <= end) is issued, ev_main[m] is recorded on the main stream and
 * ev_side[m] on the side stream (hipEvent_t handles from salt_event_create).  The data-parallel backward (one process per GPU, replaces
 * nn.DataParallel of models.py:81-85) learns this way that an all-reduce bucket's gradients are final WITHOUT cutting the program into
 * one call per bucket (each cut cost a flush of the pending side-stream entries and the completion-signal fork hand-off). */
int salt_program_run_streams_marks(const salt_program_entry* entries, int begin, int end, void* main_stream, void* side_stream, int join_at_end,
                                   const int* marks, int nmarks, void* const* ev_main, void* const* ev_side);
int salt_event_create(void** event_out);            /* a hipEvent_t without timing */
int salt_event_destroy(void* event);
int salt_stream_wait_event(void* stream, void* event);
int salt_graph_capture(const salt_program_entry* entries, int n, void* stream, void** graph_exec_out);
/* whole-step capture: every salt_program_run* call between begin and end on `stream` (and on the side stream the two-stream executor
 * forks to) is recorded instead of executed; `stream` must not be the default stream */
int salt_graph_begin(void* stream);
int salt_graph_end(void* stream, void** graph_exec_out);
int salt_graph_launch(void* graph_exec, void* stream);
int salt_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------ classifier head (architectures/misc.py:70-71,80):
 * nn.Sequential(nn.AvgPool2d(8), nn.Conv2d(C, K, 1)) of EmptinessClassifier in one launch.  OH = H / 8, OW = W / 8 (floor; rows and
 * columns beyond 8 OH / 8 OW belong to no window):
 *   pooled[b,oh,ow,c] = (1/64) sum of the 8x8 window of x          (stored fp32)
 *   logits[b,j,oh,ow] = bias[j] + sum_c w[j][c] pooled[b,oh,ow,c]   (stored fp32 NCHW)
 * Both sums (and gw / gb of the backward call) are carried in fp64 and rounded once: a logit may cancel far below its terms.
 * H < 8 or W < 8 is SALT_E_BADARG. */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,C], may be a channel slice */
    const float* w;           /* [K][C] fp32 (the module's [K,C,1,1] weight in place) */
    const float* bias;        /* [K] or NULL */
    int K;                    /* 1 .. 8 */
    float* logits_nchw;       /* out fp32 [B,K,OH,OW] */
    float* pooled;            /* out fp32 [B,OH,OW,C] kept for salt_pool_head_bwd, or NULL (eval) */
} salt_pool_head_args;
int salt_pool_head(const salt_pool_head_args*, void* stream);

/* dx[b,h,w,c] (+)= (1/64) sum_j w[j][c] dlogits[b,j,h/8,w/8] inside the windows; outside them accumulate = 0 writes zero and
 * accumulate = 1 leaves the pixel alone.  gw[j][c] = sum_{b,oh,ow} dlogits pooled and gb[j] = sum dlogits are OVERWRITTEN (as
 * salt_head1x1_bwd does), summed in ascending (b, oh, ow) order: the same bits on every run.  x itself is not read. */
typedef struct {
    int dtype;
    salt_view dx;             /* gradient view of the forward input [B,H,W,C]; p == NULL: no data gradient (the shape is still read) */
    const float* w;           /* [K][C] */
    int K;
    const float* dlogits_nchw; /* fp32 [B,K,OH,OW] */
    const float* pooled;      /* fp32 [B,OH,OW,C] from the forward call */
    int accumulate;           /* dx += */
    float* gw;                /* out [K][C] */
    float* gb;                /* out [K] or NULL */
} salt_pool_head_bwd_args;
int salt_pool_head_bwd(const salt_pool_head_bwd_args*, void* stream);

/* ------------------------------------------------------------------ second-level (stacking) network (architectures/misc.py:8-36):
 * Conv2dBnRelu(M, F, (3,3)) with the replicate-top-2 / replicate-right-2 pad (base.py:26) straight from the fp32 NCHW stack
 * [B,M,H,W] of first-level probability maps, on the matrix cores, with one of two epilogues:
 *   conv[b,y,x,f] = bias[f] + sum_{m,kh,kw} w[f][m][kh][kw] x[b,m,max(y+kh-2,0),min(x+kw,W-1)]      (x rounded to `dtype` first)
 *   train form (y.p != NULL):  y = conv (raw, NHWC, `dtype`); stats / stats_cnt = per-tile (sum, M2 about the tile's own mean,
 *       count) of the STORED y, tile < salt_stack_conv_stats_parts (salt_bn_finalize's protocol, fixed order: no atomics);
 *       xs[b,y,x,0..Mpad) = x as NHWC in `dtype`, Mpad = M rounded up to 16, channels >= M zero (Q of the weight gradient)
 *   eval form (logits_nchw != NULL):  a = relu?(conv * scale + shift) * gate[b][f];  logits[b,k,y,x] = head_b[k] + sum_f head_w[k][f] a
 *       (fp32 NCHW; nothing else is written)
 * 1 <= M <= 64, F in {16, 32, 64}, K <= 4, any H, W >= 1; anything else is SALT_E_UNSUPPORTED.  x is never written. */
typedef struct {
    int dtype;
    const float* x;           /* fp32 NCHW [B,M,H,W] */
    int B;
    int M;
    int H;
    int W;
    const float* w;           /* fp32 master weight [F][M][3][3] */
    const float* bias;        /* [F] or NULL */
    int F;
    salt_view y;              /* train form: [B,H,W,F], 16-byte aligned, cs a multiple of 4 (f32) / 8 (bf16) */
    salt_view xs;             /* train form: [B,H,W,Mpad], same alignment rules */
    float* stats;             /* train form: [nparts][2][F] (sized by salt_bn_stats_floats) */
    float* stats_cnt;         /* train form: [nparts] */
    const float* scale;       /* eval form: folded BatchNorm [F], or both NULL */
    const float* shift;
    int relu;
    const float* gate;        /* eval form: [B][gate_cs] per-image channel gate (channels 0 .. F-1 of each row), or NULL */
    int gate_cs;
    const float* head_w;      /* eval form: [K][F] fp32 (the head's [K,F,1,1] weight in place) */
    const float* head_b;      /* [K] or NULL */
    int K;
    float* logits_nchw;       /* eval form: out fp32 [B,K,H,W] */
} salt_stack_conv_args;
int salt_stack_conv(const salt_stack_conv_args*, void* stream);
int salt_stack_conv_stats_parts(const salt_stack_conv_args*);   /* < 0: unsupported shape (salt_last_error says why) */

/* grad[f][m][kh][kw] (+)= gpad[f][m][kh][kw], m < M, of a weight gradient reduced over the padded channels ([F][Mpad][3][3]) */
typedef struct {
    const float* gpad;
    int F;
    int M;
    int Mpad;
    float* grad;              /* [F][M][3][3] */
    int accumulate;
} salt_stack_grad_unfold_args;
int salt_stack_grad_unfold(const salt_stack_grad_unfold_args*, void* stream);

/* ------------------------------------------------------------------ SE-ResNet bottleneck tail (csrc/se_res.hip): the end of
 * SEResNetBottleneck.forward of the public pretrainedmodels senet.py (reached through architectures/encoders.py:48-83), restated:
 *   z[b,h,w,c]  = in_scale[c] x + in_shift[c]                (x: the raw conv3 output; both NULL: z = x, BatchNorm already applied)
 *   gap[b,c]    = mean_hw z = in_scale[c] mean_hw(x) + in_shift[c]   (the pooling pass reads raw x only)
 *   hidden[b,r] = relu(b1[r] + sum_c w1[r][c] gap[b,c]),   gate[b,c] = sigmoid(b2[c] + sum_r w2[c][r] hidden[b,r])
 *   y           = relu(gate[b,c] z + res)
 * Three launches: pooling (per-workgroup sums -> ONE fp64 atomic per channel into gap_acc, or one partial row per workgroup), the FC
 * (one workgroup per image, w1 / w2 streamed from global memory), the apply pass.  C a multiple of 64 up to 2048, R = C / 16, any
 * B, H, W >= 1; x / res / y 16-byte aligned with cs a multiple of 4 (f32) / 8 (bf16), fewer than 2^31 elements per view: anything
 * else is SALT_E_UNSUPPORTED.
 * Sums: gap_acc != NULL: [B][C] fp64, zeroed by the caller before the call (the statistics arena); else gap_partials
 * [B][nparts][C] fp32, added in ascending part order by the FC launch (the same bits on every run). */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,C] raw convolution output (or the stored BatchNorm output when in_scale == NULL) */
    const float* in_scale;    /* [C] or NULL (with in_shift) */
    const float* in_shift;
    /* consumer-side finalize of the train-mode BatchNorm in front (the protocol of salt_scse_args.in_fin): in_fin = the layer's const
     * salt_bn_finalize_args*, in_fin_acc = the [8][2 C + 1] fp64 shards the convolution launch added x's statistics to.  The FC launch
     * finalizes them (workgroup 0 stores mean / invstd / scale / shift / running statistics) and in_scale / in_shift are ignored:
     * the apply pass and salt_se_res_bwd read the stored scale / shift. */
    const void* in_fin;
    const double* in_fin_acc;
    salt_view res;            /* shortcut [B,H,W,C] */
    const float* w1;          /* [R][C]  (se_module.fc1.weight, a [R,C,1,1] convolution weight in place) */
    const float* b1;          /* [R] */
    const float* w2;          /* [C][R]  (se_module.fc2.weight) */
    const float* b2;          /* [C] */
    int R;                    /* C / 16 */
    float* gap_partials;      /* [B][nparts][C] workspace, or NULL with gap_acc */
    int nparts;               /* as returned by salt_se_res_parts */
    double* gap_acc;          /* [B][C] zeroed fp64 sums, or NULL */
    float* gap;               /* out [B][C]  (kept for salt_se_res_bwd / salt_se_res_fc_grads) */
    float* hidden;            /* out [B][R] */
    float* gate;              /* out [B][C] */
    salt_view y;              /* out [B,H,W,C] */
} salt_se_res_args;
int salt_se_res(const salt_se_res_args*, void* stream);
int salt_se_res_parts(const salt_se_res_args*);      /* pixel parts per image (x's shape and dtype are read); < 0: unsupported shape */

/* Backward of the tail.  m = dy [y > 0]:
 *   dres (+)= m;   dgate[b,c] = sum_hw m z   (z recomputed from x as above; per-workgroup sums -> `acc` [B][C] zeroed fp64, or
 *   `partials` [B][nparts][C] added in ascending order: two runs are then bit-identical)
 *   du = dgate gate (1 - gate);  dh[b,r] = [hidden > 0] sum_c du[b,c] w2[c][r];  dgap[b,c] = (1 / HW) sum_r dh[b,r] w1[r][c]
 *   dx = m gate[b,c] + dgap[b,c]          (dL/dz: the BatchNorm backward of the layer in front runs on it; dx may alias dy)
 * du, dh and dgap are stored ([B][C], [B][R], [B][C] fp32) and salt_se_res_fc_grads (same struct, any stream ordered behind this
 * call) OVERWRITES g_w2 = du^T hidden, g_b2 = sum_b du, g_w1 = dh^T gap, g_b1 = sum_b dh, images in ascending order.
 * defer_param_grads = 0: salt_se_res_bwd runs that launch itself. */
typedef struct {
    int dtype;
    salt_view x;              /* as in the forward call */
    const float* in_scale;    /* [C] scale / shift the forward call used (in_fin: the layer's stored scale / shift), or both NULL */
    const float* in_shift;
    salt_view y;              /* forward output (ReLU mask) */
    salt_view dy;             /* dL/dy */
    const float* w1;
    const float* w2;
    int R;
    const float* gap;         /* from the forward call */
    const float* hidden;
    const float* gate;
    float* partials;          /* [B][nparts][C] workspace, or NULL with acc */
    int nparts;
    double* acc;              /* [B][C] zeroed fp64 sums, or NULL */
    float* du;                /* workspace / out [B][C] */
    float* dh;                /* workspace / out [B][R] */
    float* dgap;              /* workspace / out [B][C] */
    salt_view dx;             /* out dL/dz [B,H,W,C] */
    salt_view dres;           /* dL/dres */
    int accumulate_dres;      /* dres += */
    float* g_w1;              /* out [R][C] */
    float* g_b1;              /* out [R] */
    float* g_w2;              /* out [C][R] */
    float* g_b2;              /* out [C] */
    int defer_param_grads;    /* 1: g_* are left to salt_se_res_fc_grads */
} salt_se_res_bwd_args;
int salt_se_res_bwd(const salt_se_res_bwd_args*, void* stream);
int salt_se_res_fc_grads(const salt_se_res_bwd_args*, void* stream);

/* ------------------------------------------------------------------ grouped 3x3 convolution (csrc/conv_group.hip): conv2 of
 * SEResNeXtBottleneck in the public pretrainedmodels senet.py (reached through architectures/encoders.py:86-118), restated:
 * nn.Conv2d(C, C, 3, stride, padding 1, groups 32, bias=False).  With Cg = C / 32, g = n / Cg:
 *   conv[b,oy,ox,n] = sum_{k < Cg, kh, kw} w[n][k][kh][kw] x[b, oy stride + kh - 1, ox stride + kw - 1, g Cg + k]   (zero outside x)
 * on [B,OH,OW,C], OH = (H - 1) / stride + 1 (floor; odd maps are legal).  The kernels read the fp32 master weight [C][Cg][3][3]
 * directly - there is no packed copy - and contract in fp32 on the vector ALU with the true Cg (36 .. 288 multiply-adds per output).
 * C in {128, 256, 512, 1024}, groups 32, stride 1 | 2, any B, H, W >= 1; views 16-byte aligned with cs a multiple of 4 (f32) / 8
 * (bf16); anything else is SALT_E_UNSUPPORTED / SALT_E_BADARG with a salt_last_error text (the shape rule needs no GPU).
 *   eval  (stats == NULL and fin_acc == NULL):  y = relu?(conv scale[n] + shift[n])      (scale / shift both NULL: y = relu?(conv))
 *   train (stats or fin_acc, never both; scale / shift NULL, relu 0):  y = conv, and the BatchNorm statistics of the STORED y:
 *       stats / stats_cnt: per-tile (sum, M2 about the tile's own mean, count), tile < salt_gconv_stats_parts, fixed order, no
 *           atomics (salt_bn_finalize's protocol);
 *       fin_acc: [8][2 C + 1] fp64 shards (sum, sum of squares, count), shard = workgroup id % 8, added with fp64 atomics and NO
 *           ticket: the consumer finalizes (salt_conv_args.fin_acc without fin_ticket).  Zero before the launch (salt_zero). */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,C], may be a channel slice */
    const float* w;           /* fp32 master weight [C][C / groups][3][3] */
    int groups;               /* 32 */
    int stride;               /* 1 | 2 */
    salt_view y;              /* out [B,OH,OW,C] */
    const float* scale;       /* eval: folded BatchNorm [C], or both NULL */
    const float* shift;
    int relu;
    float* stats;             /* train, partials: [nparts][2][C] (sized by salt_bn_stats_floats) */
    float* stats_cnt;         /* [nparts] */
    double* fin_acc;          /* train, shards: [8][2 C + 1] */
} salt_gconv_args;
int salt_gconv(const salt_gconv_args*, void* stream);
int salt_gconv_stats_parts(const salt_gconv_args*);   /* x's shape, groups and stride are read; < 0: unsupported shape */

/* dx[b,iy,ix,g Cg + k] (+)= sum_{n in group g, kh, kw} w[n][k][kh][kw] dy[b,oy,ox,n] over the (oy, ox) with oy stride + kh - 1 = iy,
 * ox stride + kw - 1 = ix: the gather form - with stride 2 an input pixel takes only the taps of its own parity, in ONE launch.
 * accumulate follows Act.grad_state(): 0 overwrites every element of dx, 1 adds to the stored value (one more storage rounding). */
typedef struct {
    int dtype;
    salt_view dy;             /* [B,OH,OW,C] */
    const float* w;           /* [C][C / groups][3][3] */
    int groups;
    int stride;
    salt_view dx;             /* out [B,H,W,C]; OH = (H - 1) / stride + 1 is checked against dy */
    int accumulate;
} salt_gconv_dgrad_args;
int salt_gconv_dgrad(const salt_gconv_dgrad_args*, void* stream);

/* grad[n][k][kh][kw] (+)= sum_{b,oy,ox} dy[b,oy,ox,n] x[b, oy stride + kh - 1, ox stride + kw - 1, g Cg + k]: the reference layout
 * [C][Cg][3][3].  Two launches of one entry point: nsplit = salt_gconv_wgrad_parts pixel splits write partial slabs
 * [nsplit][C][Cg][3][3] (fixed summation order inside a split), the second launch adds them in ascending split order - no atomics,
 * the same bits on every run. */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,C] forward input */
    salt_view dy;             /* [B,OH,OW,C] */
    int groups;
    int stride;
    float* partials;          /* workspace [nsplit][C][Cg][3][3] fp32 */
    int nsplit;               /* as returned by salt_gconv_wgrad_parts */
    float* grad;              /* out [C][Cg][3][3] */
    int accumulate;           /* grad += */
} salt_gconv_wgrad_args;
int salt_gconv_wgrad(const salt_gconv_wgrad_args*, void* stream);
int salt_gconv_wgrad_parts(const salt_gconv_wgrad_args*);   /* x's shape, groups and stride are read; < 0: unsupported shape */

/* ------------------------------------------------------------------ pre-activated 1x1 convolution (csrc/dense.hip): conv1 of a
 * DenseNet layer and the convolution of a transition in the public torchvision / pretrainedmodels densenet.py (reached through
 * architectures/encoders.py:121-164), restated: conv(relu(norm(x))) with nn.Conv2d(Cin, Cout, 1, bias=False), where x is a channel
 * prefix of the block's concatenation buffer and norm is a BatchNorm the CONSUMER owns.  The normalised copy of x is never stored:
 * the loader applies the transform between the global load and the matrix-core operand.
 *
 * THE INPUT TRANSFORM IS PINNED, bit for bit, for all three operators:
 *     t(x)  = fmaf(x, in_scale[c], in_shift[c])        one fused multiply-add in fp32 (x widened exactly from its storage type)
 *     a(x)  = round_to_dtype(max(0, t(x)))             one rounding to nearest even to the storage type (identity for SALT_F32)
 *     m(x)  = [t(x) > 0]
 * A float64 multiply-add of bf16-representable operands, rounded once to fp32, reproduces t exactly; a mask that flipped on a
 * near-zero t would change the data gradient by a whole value, so reference and kernel must agree on this rule.
 *
 * Shapes: Cin a multiple of 32 in [32, 2048], Cout a multiple of 64 in [64, 1024], any B, H, W >= 1 (the GEMM is M = B H W pixels,
 * K = Cin, N = Cout); anything else is SALT_E_UNSUPPORTED with a salt_last_error text, nothing is launched, and a *_parts query
 * returns < 0.  Views are 16-byte aligned with cs a multiple of 4 (f32) / 8 (bf16) and C <= cs; w, in_scale and in_shift are 16-byte
 * aligned (SALT_E_BADARG otherwise).
 * Weights: the kernels read the fp32 MASTER weight [Cout][Cin] directly - no packed copy, nothing to refresh after an optimizer step.
 * SALT_BF16 rounds it to bf16 (nearest even) on the way into LDS and contracts with v_mfma_f32_32x32x16_bf16, fp32 accumulation;
 * SALT_F32 contracts with the exact-f32 v_mfma_f32_32x32x2_f32, as salt_conv does.
 *
 *   v[p,n] = sum_c W[n][c] a(x[p,c])
 *   eval  (stats == NULL):  y = relu?(v scale[n] + shift[n])     (scale / shift both NULL: y = relu?(v); a transition passes neither)
 *   train (stats != NULL; scale / shift NULL, relu 0):  y = v and the BatchNorm statistics of the STORED y as per-tile partials
 *       (sum, M2 about the tile's own mean, count), tile < salt_dense_conv_stats_parts, fixed order, no atomics: salt_bn_finalize's
 *       protocol, the same bits on every run. */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,Cin] raw input, may be a channel prefix / slice of a wider buffer */
    const float* in_scale;    /* [Cin] */
    const float* in_shift;    /* [Cin] */
    const float* w;           /* fp32 master weight [Cout][Cin] */
    salt_view y;              /* out [B,H,W,Cout] */
    const float* scale;       /* eval: folded BatchNorm of the OUTPUT [Cout], or both NULL */
    const float* shift;
    int relu;
    float* stats;             /* train: [nparts][2][Cout] (sized by salt_bn_stats_floats) */
    float* stats_cnt;         /* [nparts] */
} salt_dense_conv_args;
int salt_dense_conv(const salt_dense_conv_args*, void* stream);
int salt_dense_conv_stats_parts(const salt_dense_conv_args*);   /* x's shape and y.C are read; < 0: unsupported shape */

/* Data gradient of the operator above INCLUDING the backward of the train-mode BatchNorm in front of it (norm, with batch statistics
 * mean / invstd of x and weight gamma).  With g[p,c] = m(x[p,c]) sum_n W[n][c] dy[p,n], N = B H W, xhat = (x - mean[c]) invstd[c]:
 *     dbeta[c]  = sum_p g[p,c]            dgamma[c] = sum_p g[p,c] xhat[p,c]
 *     dx[p,c] (+)= gamma[c] invstd[c] (g - dbeta[c] / N - xhat dgamma[c] / N)
 * Three launches of one entry point: the contraction with the two sums reduced per 128-pixel tile into `partials` (fixed order), a
 * finalize launch that adds the tiles in ascending order (fp64, rounded once) into `sums` and dgamma / dbeta, and the contraction
 * again with the apply in its epilogue.  g is RECOMPUTED, not stored: the second pass reads dy once more (M Cout elements) where a
 * stash would write and read M Cin elements, Cin >= Cout / 2 ... 8 Cout in a DenseNet; both passes run the same instructions, so
 * they see the same g.  accumulate: 0 overwrites dx, 1 adds to the stored value (one more storage rounding). */
typedef struct {
    int dtype;
    salt_view dy;             /* [B,H,W,Cout] */
    const float* w;           /* fp32 master weight [Cout][Cin] */
    salt_view x;              /* [B,H,W,Cin] forward input */
    const float* in_scale;    /* [Cin] forward transform (mask) */
    const float* in_shift;
    const float* mean;        /* [Cin] batch statistics of x */
    const float* invstd;
    const float* gamma;       /* [Cin] weight of norm */
    float* partials;          /* workspace [nparts][2][Cin] fp32 */
    int nparts;               /* as returned by salt_dense_conv_dgrad_parts */
    float* sums;              /* workspace [2][Cin]: this launch's dbeta, dgamma */
    float* dgamma;            /* out [Cin] */
    float* dbeta;             /* out [Cin] */
    int accumulate_param_grads;   /* dgamma / dbeta += */
    salt_view dx;             /* out [B,H,W,Cin] */
    int accumulate;           /* dx += */
} salt_dense_conv_dgrad_args;
int salt_dense_conv_dgrad(const salt_dense_conv_dgrad_args*, void* stream);
int salt_dense_conv_dgrad_parts(const salt_dense_conv_dgrad_args*);   /* x's shape and dy.C are read; < 0: unsupported shape */

/* grad[n][c] (+)= sum_p dy[p,n] a(x[p,c]) in the master weight's layout [Cout][Cin], the same pinned transform in the loader.
 * nsplit = salt_dense_conv_wgrad_parts pixel splits write partial slabs [nsplit][Cout][Cin] (fixed order inside a split), a second
 * launch adds them in ascending split order - no atomics, the same bits on every run. */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,Cin] forward input */
    const float* in_scale;    /* [Cin] */
    const float* in_shift;
    salt_view dy;             /* [B,H,W,Cout] */
    float* partials;          /* workspace [nsplit][Cout][Cin] fp32 */
    int nsplit;               /* as returned by salt_dense_conv_wgrad_parts */
    float* grad;              /* out [Cout][Cin] */
    int accumulate;           /* grad += */
} salt_dense_conv_wgrad_args;
int salt_dense_conv_wgrad(const salt_dense_conv_wgrad_args*, void* stream);
int salt_dense_conv_wgrad_parts(const salt_dense_conv_wgrad_args*);   /* x's shape and dy.C are read; < 0: unsupported shape */

/* Per-channel moments of a STORED view (the stem output or a pooled transition output that opens a dense block): per-tile partials
 * (sum, M2 about the tile's own mean, count) over 128-pixel tiles in salt_bn_finalize's protocol, fixed order, no atomics.  No other
 * operator can supply them: salt_conv reports the statistics of a raw convolution output only, and these channels are the output of
 * an activation / a pooling pass.  Any C >= 1, any view. */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,C], may be a channel slice */
    float* stats;             /* [nparts][2][C] (sized by salt_bn_stats_floats) */
    float* stats_cnt;         /* [nparts] */
} salt_dense_moments_args;
int salt_dense_moments(const salt_dense_moments_args*, void* stream);
int salt_dense_moments_parts(const salt_dense_moments_args*);   /* x's shape is read; < 0: unsupported shape */

/* One statistics table per dense block: channel c of the concatenation buffer has ONE batch mean / variance, whichever later layer
 * normalises it (the data is identical, only gamma / beta differ).  The table (mean, invstd, unbiased variance per channel) is filled
 * once, when the channels are produced (salt_bn_finalize with gamma 1, beta 0, momentum 1 on the producer's partials); every layer
 * then derives its own coefficients for its channel prefix and updates its own running statistics, with salt_bn_finalize's arithmetic:
 *     in_scale = gamma invstd      in_shift = beta - mean in_scale
 *     running_mean = (1 - momentum) running_mean + momentum mean      running_var likewise with the unbiased variance
 *     num_batches_tracked += 1
 * so that a layer's state_dict comes out as if it had computed the statistics itself. */
typedef struct {
    int C;
    const float* mean;        /* [C] the block's table */
    const float* invstd;
    const float* unbiased_var;
    const float* gamma;       /* [C] the layer's BatchNorm */
    const float* beta;
    float* running_mean;      /* [C] or both NULL */
    float* running_var;
    int64_t* num_batches_tracked;   /* or NULL */
    float momentum;
    float* in_scale;          /* out [C] */
    float* in_shift;          /* out [C] */
} salt_dense_bn_prep_args;
int salt_dense_bn_prep(const salt_dense_bn_prep_args*, void* stream);

/* ------------------------------------------------------------------ paired line convolution (csrc/gcn.hip): the entry of the reference's
 * GlobalConvolutionalNetwork (architectures/base.py:152-178).  conv1[0] (K x 1) and conv2[0] (1 x K) read the same encoder map x, the only
 * wide tensor of the block; both pad one-sided by replication (Conv2dBnRelu: K - 1 rows on top, K - 1 columns on the right):
 *     yv[b,i,j,n] = epi_v( sum_k sum_c wv[n][c][k] x[b, max(i - (K-1) + k, 0), j, c] )
 *     yh[b,i,j,n] = epi_h( sum_k sum_c wh[n][c][k] x[b, i, min(j + k, W - 1), c] )
 * ONE launch stages an L-shaped region of x per 8 x 16 pixel tile (rows i0 - (K-1) .. i0 + 7 of the tile's columns, then the K - 1
 * columns to its right for the tile's rows) and contracts it for both branches.  The clamp is in the loader: no padded copy.
 *
 * Shapes: Cin a multiple of 8 up to 2048; Cout 1 .. 32, the same for both branches; K 2 .. 9 (even K is legal: the pad is one-sided);
 * any B, H, W >= 1, H or W below K - 1 included.  x, yv, yh are 16-byte aligned NHWC views with cs >= C a multiple of 4 (f32) / 8 (bf16),
 * channel slices of wider buffers included.  Anything else is SALT_E_UNSUPPORTED with a salt_last_error text, nothing is launched and
 * salt_gcn_pair_stats_parts returns < 0 (it reads the struct on the host only).
 * Weights: the fp32 MASTER weights, conv.weight of shape [Cout,Cin,K,1] / [Cout,Cin,1,K] = [Cout][Cin][K] in memory - no packed copy,
 * nothing to refresh after an optimizer step.  SALT_BF16 rounds them to bf16 (nearest even) on the way into LDS and contracts with
 * v_mfma_f32_32x32x16_bf16 (Cout padded to the 32-wide tile with zero rows), fp32 accumulation; SALT_F32 contracts with the exact-f32
 * v_mfma_f32_32x32x2_f32, as salt_conv does.
 *   eval  (no stats):  epi(v) = relu?((v + bias[n]) * scale[n] + shift[n]), each part optional per branch (scale / shift go together)
 *   train (stats_v, stats_cnt_v, stats_h, stats_cnt_h all set; no scale / shift / relu):  y = v + bias and the BatchNorm statistics of
 *       the STORED y as per-tile partials (sum, M2 about the tile's own mean, count), tile < salt_gcn_pair_stats_parts, in
 *       salt_bn_finalize's layout [nparts][2][Cout] / [nparts] (sized by salt_bn_stats_floats), fixed order, no atomics: the same bits
 *       on every run. */
typedef struct {
    int dtype;
    salt_view x;              /* [B,H,W,Cin], may be a channel slice */
    const float* wv;          /* fp32 master weight of the K x 1 convolution [Cout][Cin][K] */
    const float* wh;          /* fp32 master weight of the 1 x K convolution [Cout][Cin][K] */
    int K;
    salt_view yv;             /* out [B,H,W,Cout] */
    salt_view yh;             /* out [B,H,W,Cout] */
    const float* bias_v;      /* [Cout] or NULL */
    const float* scale_v;     /* eval: folded BatchNorm [Cout], or both NULL */
    const float* shift_v;
    int relu_v;
    const float* bias_h;
    const float* scale_h;
    const float* shift_h;
    int relu_h;
    float* stats_v;           /* train: [nparts][2][Cout] */
    float* stats_cnt_v;       /* [nparts] */
    float* stats_h;
    float* stats_cnt_h;
} salt_gcn_pair_args;
int salt_gcn_pair(const salt_gcn_pair_args*, void* stream);
int salt_gcn_pair_stats_parts(const salt_gcn_pair_args*);   /* host only: the shapes, K and the alignment are read; < 0: unsupported */

/* The gradient of x from BOTH branches in one launch that writes dx once (a plain store, or += with accumulate): no extended grid, no
 * fold ring, no strip, no second pass.  The adjoint of the one-sided clamp, checked in float64 against autograd:
 *     dx[b,r,j,c] = sum_k wv[:,c,k]^T dyv[b, r + (K-1) - k, j]            (rows outside [0, H) contribute nothing)
 *                 + sum_k wh[:,c,k]^T dyh[b, r, j - k]                    (columns outside [0, W) contribute nothing)
 *                 + [r == 0]     sum_{i <= min(K-2, H-1)} sum_{k <= K-2-i} wv[:,c,k]^T dyv[b, i, j]
 *                 + [j == W - 1] sum_{j' >= max(W-K+1, 0)} sum_{k >= W-j'} wh[:,c,k]^T dyh[b, r, j']
 * THE SUMMATION ORDER IS FIXED (fp32 accumulation; a rerun gives the same bits), per element of dx:
 *     1. the K x 1 taps, k = 0 .. K-1;
 *     2. row 0 only: its clamp taps, k = 0 .. K-2 and inside a k the source row i = K-2-k down to 0;
 *     3. the 1 x K taps, k = 0 .. K-1;
 *     4. column W - 1 only: its clamp taps, k = 1 .. K-1 and inside a k the source column j' = W-k .. W-1;
 *     inside a tap the matrix core's order over the output channels; then the stored dx is added when accumulate is set.
 * The clamp taps are ordinary taps on the ORIGINAL weights (one per (k, source) pair, which is the prefix- / suffix-summed weight of
 * the formula applied term by term): no summed weight is rounded to bf16.  Shapes, views, dtypes and weights as above (dx in x's role). */
typedef struct {
    int dtype;
    salt_view dyv;            /* [B,H,W,Cout] */
    salt_view dyh;            /* [B,H,W,Cout] */
    const float* wv;          /* fp32 master weights, as in the forward call */
    const float* wh;
    int K;
    salt_view dx;             /* out [B,H,W,Cin] */
    int accumulate;           /* dx += */
} salt_gcn_pair_dgrad_args;
int salt_gcn_pair_dgrad(const salt_gcn_pair_dgrad_args*, void* stream);

/* ------------------------------------------------------------------ pyramid pooling at low resolution (csrc/psp.hip): the middle of
 * the reference's PSPNet (architectures/pspnet.py: PSPModule, PSPUpsample).  PSPModule pools its input x [B,h,w,C] to s x s bins for every
 * pyramid size s, runs a 1x1 convolution per size, resizes the results back to h x w, concatenates them with x and runs the 1x1
 * `bottleneck` + ReLU over the 5 C channels.  A 1x1 convolution commutes with the bilinear resize, so with W_b = bottleneck.weight in
 * input-channel blocks (the stages in order, then x):
 *     q_k = W_b[:, k C : (k + 1) C] (W_k pool_k(x))        at s_k x s_k
 *     f   = W_b[:, n C : (n + 1) C] x                      at h x w
 *     y   = relu(f + bias + sum_k resize_{s_k -> (h, w)}(q_k))
 * The contractions are salt_conv launches on weight slices; the operators here are what is left: the pooling, the merge and their
 * adjoints, and PSPUpsample's BatchNorm apply + PReLU.
 *
 * Shapes of the four psp operators: h, w <= 32; C a multiple of 8 (both dtypes); 1..4 pyramid sizes, each in 1..6; every view 16-byte
 * aligned with cs a multiple of 4 (f32) / 8 (bf16), channel slices of wider buffers included.  Anything else is SALT_E_UNSUPPORTED /
 * SALT_E_BADARG with a salt_last_error text and nothing is launched.  All sums are fp32 in a fixed order, no atomics: a rerun gives
 * the same bits.  Stage k of a pooled tensor is a view [B, s_k, s_k, C] of its own.
 *
 * Bins follow torch's AdaptiveAvgPool2d: rows [floor(i h / s), ceil((i + 1) h / s)), columns likewise; bins overlap where s does not
 * divide h and repeat pixels where s > h.  p_k[b,i,j,c] = (sum of the window's pixels in row-major order) / area. */
#define SALT_PSP_MAX_STAGES 4
typedef struct {
    int dtype;
    salt_view x;              /* [B,h,w,C] */
    int nsizes;
    int sizes[SALT_PSP_MAX_STAGES];
    salt_view p[SALT_PSP_MAX_STAGES];   /* out: stage k [B,s_k,s_k,C] */
} salt_psp_pool_args;
int salt_psp_pool(const salt_psp_pool_args*, void* stream);

/* dx[b,y,x,c] (+)= sum_k sum_{bins of stage k that contain (y, x)} dp_k[bin] / area(bin): a gather per pixel - stages, bin rows, bin
 * columns ascending. */
typedef struct {
    int dtype;
    int nsizes;
    int sizes[SALT_PSP_MAX_STAGES];
    salt_view dp[SALT_PSP_MAX_STAGES];  /* stage k [B,s_k,s_k,C] */
    salt_view dx;             /* out [B,h,w,C] */
    int accumulate;           /* dx += */
} salt_psp_pool_bwd_args;
int salt_psp_pool_bwd(const salt_psp_pool_bwd_args*, void* stream);

/* y = relu(f + bias + sum_k resize(q_k)).  The resize is torch's size-based bilinear interpolation (F.upsample(size=(h, w),
 * mode='bilinear')), source index of destination d along an axis of n destinations and s sources, PINNED in fp32:
 *     align_corners 0:  src = max(0, (s / n) (d + 0.5) - 0.5)          align_corners 1:  src = ((s - 1) / (n - 1)) d   (0 for n = 1)
 *     i0 = min(int(src), s - 1)    i1 = min(i0 + 1, s - 1)    w1 = src - i0    w0 = 1 - w1
 * one division, one product and one subtraction, each rounded once.  A tap's weight is the rounded product of its row and column
 * weight. */
typedef struct {
    int dtype;
    salt_view f;              /* [B,h,w,C] */
    const float* bias;        /* [C] or NULL */
    int nsizes;
    int sizes[SALT_PSP_MAX_STAGES];
    salt_view q[SALT_PSP_MAX_STAGES];   /* stage k [B,s_k,s_k,C] */
    int align_corners;
    salt_view y;              /* out [B,h,w,C] */
} salt_psp_merge_args;
int salt_psp_merge(const salt_psp_merge_args*, void* stream);

/* From dy and the stored y:  g = dy [y > 0] -> df (df may be dy itself);  dq_k[bin] = sum_pixels weight_k(pixel, bin) g[pixel], a gather
 * per bin with the pixels in row-major order (weight_k: the dense resize matrix, a source that both taps of a clamped destination hit
 * gets the rounded sum w0 + w1);  dbias[c] (+)= sum_b partials[b][c], partials[b][c] = sum_pixels g[b,pixel,c], images ascending. */
typedef struct {
    int dtype;
    salt_view dy;             /* [B,h,w,C] */
    salt_view y;              /* [B,h,w,C] forward output */
    int nsizes;
    int sizes[SALT_PSP_MAX_STAGES];
    int align_corners;
    salt_view df;             /* out [B,h,w,C] */
    salt_view dq[SALT_PSP_MAX_STAGES];  /* out: stage k [B,s_k,s_k,C] */
    float* partials;          /* workspace [nparts][C] fp32 */
    int nparts;               /* as returned by salt_psp_merge_bwd_parts */
    float* dbias;             /* out [C], or NULL */
    int accumulate_dbias;     /* dbias += */
} salt_psp_merge_bwd_args;
int salt_psp_merge_bwd(const salt_psp_merge_bwd_args*, void* stream);
int salt_psp_merge_bwd_parts(const salt_psp_merge_bwd_args*);   /* dy's shape is read */

/* PSPUpsample's BatchNorm2d apply + nn.PReLU() (one learnable slope, read from device memory) in one pass over the raw convolution
 * output; the normalised value is never stored.  THE PRE-ACTIVATION IS PINNED for both operators:
 *     u = fmaf(y, scale[c], shift[c])     (scale == shift == NULL: u = y - the convolution's epilogue already applied a folded BatchNorm)
 *     a = u > 0 ? u : alpha u
 * Any B, H, W; C a multiple of 8; 16-byte aligned views as above.  a may be y itself. */
typedef struct {
    int dtype;
    salt_view y;              /* [B,H,W,C] */
    const float* scale;       /* [C] or NULL (then shift is NULL too) */
    const float* shift;
    const float* alpha;       /* [1] */
    salt_view a;              /* out [B,H,W,C] */
} salt_bn_prelu_args;
int salt_bn_prelu(const salt_bn_prelu_args*, void* stream);

/* du = da (u > 0 ? 1 : alpha) (du may be da itself; salt_bn_bwd with relu = 0 then runs on du);  dalpha (+)= sum da min(u, 0): every
 * workgroup reduces its share in a fixed order into partials[workgroup], a second launch adds the partials in a fixed order. */
typedef struct {
    int dtype;
    salt_view da;             /* [B,H,W,C] */
    salt_view y;              /* [B,H,W,C] raw convolution output */
    const float* scale;
    const float* shift;
    const float* alpha;
    salt_view du;             /* out [B,H,W,C] */
    float* partials;          /* workspace [nparts] fp32 */
    int nparts;               /* as returned by salt_bn_prelu_bwd_parts */
    float* dalpha;            /* out [1] */
    int accumulate_dalpha;    /* dalpha += */
} salt_bn_prelu_bwd_args;
int salt_bn_prelu_bwd(const salt_bn_prelu_bwd_args*, void* stream);
int salt_bn_prelu_bwd_parts(const salt_bn_prelu_bwd_args*);   /* y's shape and dtype are read */

#ifdef __cplusplus
}
#endif
#endif /* SALTNET_H */
