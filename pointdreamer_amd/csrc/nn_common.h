// Shared declarations of the UNet engine (row U1/D1) translation units.
#pragma once
#include "common.h"
#include <hip/hip_fp16.h>
#include <algorithm>

namespace pdnn {

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((ext_vector_type(4))) _Float16 half4;
typedef __attribute__((ext_vector_type(4))) float float4_t;

// ---- every tuning / test hook of the UNet units, with its shipped default.  The pdhip_debug_set_* entry points (nn_unet.hip) write the calling
// thread's instance; the engine's forward and route-table entry points take it once into their Ctx, the stand-alone operator entry points
// read it where they plan.  Nothing else names the instance: planners get a const Tuning&, launchers get a plan.
struct Tuning {
    // -- conv routing (conv_plan and the planners under it)
    int force_bk = 0;          // 32 / 64 forces the K-step, 0 = automatic
    int force_stages = 0;      // 2 / 3 / 4 LDS stages, 0 = automatic
    int force_wmw = 0;         // tile geometry: 2 = 128x128/4 waves, 4 = 256x128/8 waves, 8 = 256x256/8 waves, 0 = automatic
    int force_splits = 0;      // >= 1 forces the split-K factor, 0 = automatic
    int halo_strips = 0;       // pdhip_debug_set_conv_halo_strips: 0 automatic, 1 full rows (see conv_plan's halo_rows)
    int sk_mode = 1;           // pdhip_debug_set_conv_sk: 0 = never route to k_conv_sk, 1 = automatic, 2 = every eligible layer
    int sk_tile = 0;           // 0 = automatic, 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 64x32
    int sk_splits = 0;         // >= 1 forces the split factor
    int sk_stages = 0;         // lab hook: LDS stages per K-group (2, 3, 4 where the tile allows); 0 = default
    int sk_kg = 0;             // lab hook: K-groups per workgroup (1, 2, 4; 8 = loader-specialised); 0 = default
    int sk_order = 0;          // lab hook: tile order inside an XCD's run: 0 automatic, 1 pixel tiles fastest, 2 n-tiles fastest
    int rr_mode = 1;           // pdhip_debug_set_conv_rr: 0 = never, 1 = automatic, 2 = every eligible layer
    int rr_variant = 0;        // 0 = automatic, else force a variant id (see conv_rr_plan)
    int rr_slabs = 0;          // 0 = automatic, else force the slab count of the conv source
    int ht_mode = 1;           // pdhip_debug_set_conv_ht: 0 = never, 1 = automatic, 2 = every eligible layer
    int ht_slabs = 0;          //   K-slabs forced (0 = automatic)
    // -- engine folds (plan_res and its helpers, nn_unet.hip)
    // pdhip_debug_set_fuse_gn.  Default 0 = stand-alone GroupNorm-apply passes: MEASURED faster.  The in-conv
    // transform removes 9.4 ms of gn_apply per batch-32 forward but costs the halo conv 23 % (tools/bench_conv.py --apply, lab builds:
    // fetch of the staged pieces -4.5 %, the in-place ds_write_b128 -10 % -- a store occupies the SIMD's LDS path for 13 cycles in
    // front of the fragment reads the MFMAs wait for -- arithmetic -8 %): 76.2 vs 71.4 ms per DDNM step at batch 32.
    int fuse_gn = 0;
    // pdhip_debug_set_fold_resample: 1 (default) = the x branch of up / down ResBlocks is never materialised by a
    // k_resample pass: AvgPool2d(2) of the raw input comes out of the GroupNorm-apply kernel that reads the same pixels anyway, the
    // nearest x2 copy is replaced by index arithmetic in the residual read of the consuming conv (unsplit halo layers)
    int fold_resample = 1;
    // pdhip_debug_set_fold_skip: 1 (default) = where a channel-changing ResBlock's conv2 runs in k_conv_sk (the small-M
    // layers) the block's skip 1x1 conv is appended to conv2's K loop (one launch, one rounding) instead of a launch of its own + a residual read
    int fold_skip = 1;
    // pdhip_debug_set_rr_gn: largest image width at which a ResBlock conv routed to k_conv_rr also applies the GroupNorm (+ FiLM) + SiLU
    // in front of it while staging (no k_gn_apply launch, no normalised tensor; bit-identical).  Default 0 = never -- measured (profiles/r06_rr_gn_ab.txt):
    // stand-alone the 8^2 / 1024-channel conv pays +0.9 us for it (the element map runs under the weight stream) against a ~6 us launch, the 16^2 / 32^2
    // convs +9-10 us (every 16-32-channel tile redoes the map for its whole pixel tile: 100 VALU cycles per element at one wave per SIMD); inside the
    // forward the batch-1 DDNM step is 4.256 ms with it at 8^2 against 4.254-4.268 without, 4.266 at 16^2: no gain, so the two-pass form stays
    int rr_gn = 0;
    // pdhip_debug_set_fold_finalize: largest batch at which GroupNorm-apply reduces the conv epilogues' octet
    // partials itself instead of reading the output of a k_gn_finalize_oct launch (0 = never); above that batch the fold is kept for the
    // tensors whose producers left at most fold_finalize_chunks chunks per image (the 32^2 ... 8^2 levels: the re-reduction is a few
    // loads per thread against a 5.8 us launch, 2 020 of them per 20 forwards at batch 32)
    int fold_finalize = 8, fold_finalize_chunks = 16;
    // pdhip_debug_set_fuse_skip: 0 = never, 1 (default) = a channel-changing ResBlock whose skip conv is C -> 256 over
    // at least fuse_skip_min_tiles pixel tiles (default 1: measured a gain at every batch) runs GroupNorm-apply and the skip 1x1 as ONE
    // pass over its input (k_gn_skip), 2 = always
    int fuse_skip = 1, fuse_skip_min_tiles = 1;
    // pdhip_debug_set_up_phase: the in_layers conv of an up-ResBlock, conv3x3(nearest_x2(h)), as four 2x2 phase convs over the
    // half-resolution h with the coinciding taps summed in the weights (4/9 of the MACs; k_conv_igemm<4>).  0 = never, 1 (default) = where it
    // measured faster than the 9-tap route (wish_up_phase, nn_unet.hip), 2 = every eligible layer.  Independent of fold_resample.
    int up_phase = 1;
    // -- other units: handed to attention(), gn_apply() and gn_skip() as arguments by their callers
    int attn_nbuf = 0;         // 2 / 3 LDS chunk buffers of k_attention_t64, 0 = automatic
    int attn_qtn = 0;          // 1 / 2 = 64 / 128 queries per workgroup, 0 = automatic
    int attn_vt = 0;           // 1 = transposed-V workspace form (k_transpose_v + plain reads), 0 = LDS transpose reads
    int gn_iters = 0;          // lab hook (pdhip_debug_set_gn_iters): pixels per thread of k_gn_apply, 0 = default
    int gs_variant = 1;        // pdhip_debug_set_gn_skip_variant: 2 = k_gn_skip on 128-row tiles at every tile count (else 64-row tiles below 256 tiles)
};
Tuning& tuning();              // the calling thread's instance (defined once, nn_unet.hip)

// ---- implicit-GEMM convolution (nn_gemm.hip)
// X [N,H,W,Cin] f16 (NHWC), Wt [Cout_pad][TAPS*Cin] f16 (k = tap*Cin + c, tap = ky*3+kx; Cout_pad % 128 == 0),
// bias f32 [Cout] (may be null), residual [N,H,W,Cout] f16 (may be null), Y [N,H,W,Cout] f16.
// taps: 1 (1x1 conv / linear over pixels) or 9 (3x3, pad 1).  Cin % 32 == 0.
// 3x3 convolution with an LDS-resident activation halo (nn_conv_halo.hip): 512-pixel x 128-channel tiles, W in {64,128,256}
bool conv3x3_halo_eligible(int N, int H, int W, int Cin, int Cout_pad);
int conv3x3_halo_splits(int N, int H, int W, int Cin, int Cout, int Cout_pad, size_t splitk_ws_floats);   // 1 direct, >1 split, 0 = do not use
int conv3x3_halo_launch_splits(const Tuning& t, int N, int H, int W, int Cin, int Cout, int Cout_pad, size_t halo_ws_floats);   // what to launch conv3x3_halo with (>= 1; honours force_splits)
// 256-wide images: column strips of 128 (4 rows x 128 per tile: 780 halo pixels per chunk instead of 1 032) measured +2-3 %
// over full rows, strips of 64 +1.5-3 % (that instance spilled 8 VGPRs and was never the default: removed in round 5); at 128 wide
// strips do not pay.  Full rows where the hook asks for them or the height holds no whole 4-row strips.
inline bool conv3x3_halo_rows(const Tuning& t, int H, int W) { return W == 256 && (t.halo_strips == 1 || H % 4 != 0); }
// splits / full_rows: as planned (the two functions above).  gn_part (optional): GroupNorm octet partials, H*W/512 chunks per image from the direct
// epilogue, H*W/16 from the split reduce.  apply_table != NULL: the input is silu(A x + B) of X per gn_table (zero padding applies to the TRANSFORMED image)
int conv3x3_halo(const half_t* X, const half_t* Wt, const float* bias, const half_t* residual, half_t* Y, int N, int H, int W,
                 int Cin, int Cout, int Cout_pad, const half_t* zero_page, hipStream_t s, float* gn_part, int splits, bool full_rows,
                 float* splitk_ws, size_t splitk_ws_floats, const float* apply_table = nullptr, int res_up = 0,    // res_up: residual = half-resolution tensor, nearest x2 on the fly
                 int in_up = 0);                                          // in_up: X = half-resolution tensor, the conv sees its nearest x2
// fixed-order sum of split-K partials [splits][M][Cout] f32 + bias (+ residual) -> f16 Y, optional GroupNorm octet partials
int splitk_reduce(const float* partial, int splits, long long M, int Cout, const float* bias, const half_t* residual, half_t* Y,
                  float* gn_part, int hw, hipStream_t s);
// stand-alone form (the C entry points and the kernel tests): conv_plan + conv_launch, a wish the layer's kernel cannot absorb is an error
int conv_igemm(const Tuning& t, const half_t* X, const half_t* Wt, const float* bias, const half_t* residual, half_t* Y, int N, int H,
               int W, int Cin, int Cout, int Cout_pad, int taps, const half_t* zero_page, hipStream_t s,
               float* splitk_ws = nullptr, size_t splitk_ws_floats = 0, float* gn_part = nullptr,
               const half_t* X2 = nullptr, int Cin1 = 0,    // X2: second tensor of a never-materialised channel concat (1x1 only)
               const float* apply_table = nullptr,          // input = silu(A x + B) per gn_table (layers the halo kernel takes only)
               int res_up = 0,                              // residual = half-resolution tensor read with nearest x2 (unsplit halo layers only)
               int in_up = 0);                              // X = half-resolution tensor, input = its nearest x2 (halo layers only)
// ---- conv3x3(nearest_x2(X)) as four 2x2 phase convs over the half-resolution X [N,H,W,Cin] (nn_gemm.hip, k_conv_igemm<4>): Y [N,2H,2W,Cout].
// Wph [4][Cout_pad][4 Cin] from conv_up2_phase_pack(w9 = the packed [Cout_pad][9 Cin] weights); gn_part: octet partials, 4 H W / 256 chunks per image;
// geo: the tile geometry conv_up2_phase_plan chose (8 = 256x256, 16 = 256x128 / 4 waves)
bool conv_up2_phase_eligible(int N, int H, int W, int Cin, int Cout, int Cout_pad);
int conv_up2_phase_pack(const half_t* w9, int Cin, int Cout_pad, half_t* dst, hipStream_t s);
int conv_up2_phase(const half_t* X, const half_t* Wph, const float* bias, half_t* Y, int N, int H, int W, int Cin, int Cout, int Cout_pad,
                   const half_t* zero_page, hipStream_t s, float* gn_part, int geo);
// ---- small-M convolution with in-launch split-K combine (nn_conv_sk.hip).  ws: [0, 4096) ticket words (zero at allocation,
// self-resetting), slabs behind them.  conv_sk_plan decides whether / how a layer runs there (bm == 0: not this kernel's layer).
struct SkPlan { int bm, bn, splits, tile_id;
                int kg, stages, m_fast; };      // the instance: K-groups (8 / 12: loader-specialised, 4 / 8 loader waves), LDS stages (0 = the tile's default), pixel tiles fastest
SkPlan conv_sk_plan(const Tuning& t, int N, int H, int W, int Cin, int Cout, int Cout_pad, int taps, bool two_source, size_t ws_floats, int k_extra = 0);
// 3x3 conv + the ResBlock's skip 1x1 over the block input xs = [XS (Cs1 channels) | XS2 (Cs - Cs1), may be null] as ONE K loop
// (out = W2 * im2col(X) + Wskip * xs + (b2 + bskip): unet.py:255); Wt [Cout_pad][9 Cin + Cs] and bias from fuse_skip_weights
int conv_sk_skip(const SkPlan& pl, const half_t* X, const half_t* Wt, const float* bias, half_t* Y, int N, int H, int W, int Cin, int Cout,
                 int Cout_pad, const half_t* XS, const half_t* XS2, int Cs1, int Cs, const half_t* zero_page, hipStream_t s, float* ws,
                 size_t ws_floats, float* gn_part);
int fuse_skip_weights(const half_t* w3, int K9, const half_t* w1, int Cs, int Cout_pad, const float* b3, const float* b1, int Cout, half_t* dst,
                      float* bdst, hipStream_t s);
int conv_sk(const SkPlan& pl, const half_t* X, const half_t* Wt, const float* bias, const half_t* residual, half_t* Y, int N, int H, int W,
            int Cin, int Cout, int Cout_pad, int taps, const half_t* zero_page, hipStream_t s, float* ws, size_t ws_floats, float* gn_part,
            const half_t* X2, int Cin1, int res_up = 0);      // res_up: residual = half-resolution tensor read with nearest x2
#define PD_SK_TICKET_FLOATS 4096
// combine per-(chunk, channel-octet) partial sums written by the conv epilogue ([N][chunks][C/8][2]) of one tensor, or of
// the two tensors of a channel concat (A: Ca channels, B: Cb channels), into GroupNorm(32) stats [N][32][2] (mean, rstd).
int gn_finalize_oct(const float* partA, int Ca, int chunksA, const float* partB, int Cb, int chunksB, int N, int HW, float eps,
                    float* stats, hipStream_t s);

// ---- row-resident convolution of the 8^2 / 16^2 / 32^2 levels at small batch (nn_conv_rr.hip): GroupNorm (+ FiLM) (+ SiLU) of the input
// applied while staging, weights streamed HBM -> registers from a fragment-major copy, in-launch split-K over K "slabs".
struct RrIn {                      // one K source: x [N,H,W,Ca] (+ x2 [N,H,W,C-Ca]: never-materialised channel concat)
    const half_t* x; const half_t* x2; int C, Ca;
    int gn;                        // 0 raw, 1 GroupNorm, 2 GroupNorm + SiLU (statistics from the producers' octet partials, k_gn_apply's FIN arithmetic)
    const float* gamma; const float* beta; const float* film; long long film_stride;
    const float* partA; const float* partB; int chunksA, chunksB; float eps;
};
struct RrPlan { int variant, S0, U0, S1, U1, bands, ntiles; };      // variant == 0: not a layer for this kernel
RrPlan conv_rr_plan(const Tuning& t, int N, int H, int W, int Cin, int Cout, int taps, int Cs /*channels of an appended skip 1x1, 0 = none*/, size_t ws_floats,
                    bool want_gn = false /*the caller will ask for the in-staging GroupNorm: only the variants that carry it*/);
size_t conv_rr_weight_halfs(int Cin, int taps, int Cs, int Cout);
// w_packed: the engine's [Cout_pad][taps * Cin (+ Cs)] layout -> fragment-major [Cout / 16][K-steps][64 lanes][8]
int conv_rr_pack(const half_t* w_packed, int Cin, int taps, int Cs, int Cout, half_t* dst, hipStream_t s);
int conv_rr(const RrPlan& pl, const RrIn& in, const RrIn* skip, int taps, const half_t* wf, const float* bias, const half_t* residual, int res_up,
            half_t* Y, int N, int H, int W, int Cout, float* ws, size_t ws_floats, float* gn_part /*pl.bands chunks per image*/, hipStream_t s);
#define PD_RR_MAX_PART_LOADS 8    // octet-partial loads per thread of the in-kernel statistics: chunks / slots of a source must not exceed it
// The in-staging GroupNorm finishes the statistics of the groups ONE staged unit (cs channels) touches in two LDS tables of RrCfg::GN_ROWS = cs / 8 + 1 rows
// (8-channel groups at least, + 1 for a group that straddles into the unit), eight statistics threads per group: 256 threads serve at most 32 groups.
constexpr int rr_gn_groups_cap(int cs) { return cs / 8 + 1 < 32 ? cs / 8 + 1 : 32; }
// The largest group count of a unit of a C-channel GroupNorm(32) source: the kernel's own `ng` expression (k_conv_rr, issue_stats) over the units
// c0 = 0, cs, 2 cs, ... < C.  0 = not a source the kernel's magic division serves.  The plan, the launcher and the engine's wish all ask this one function.
inline int rr_gn_groups_max(int cs, int C) {
    if (cs <= 0 || C < 32 || C > 4096 || C % 32 != 0) return 0;
    const int cg = C / 32, mg = ((1 << 20) + cg - 1) / cg;           // (c0 + cs - 1 < 8192, mg <= 2^20: the products need 64 bits only where C % cs != 0)
    int worst = 0;
    for (int c0 = 0; c0 < C; c0 += cs) {
        const int g_first = (int)(((long long)c0 * mg) >> 20), ng = (int)(((long long)(c0 + cs - 1) * mg) >> 20) - g_first + 1;
        worst = std::max(worst, ng);
    }
    return worst;
}
// channels per staged unit of the variant conv_rr_plan(..., want_gn) would take for W-wide images under t's hooks (0: no variant with the in-staging GroupNorm)
int conv_rr_gn_unit(const Tuning& t, int W);

// ---- 3x3 conv on 256-pixel x 64-channel halo tiles, K unsplit (nn_conv_ht.hip): the 64^2 / 128^2 levels at batch 1-2
bool conv_ht_routes(const Tuning& t, int N, int H, int W, int Cin, int Cout, int Cout_pad, size_t ws_floats);
int conv_ht_slabs(const Tuning& t, int N, int H, int W, int Cin, int Cout_pad, size_t ws_floats);
int conv_ht(const half_t* X, const half_t* Wt, const float* bias, const half_t* residual, half_t* Y, int N, int H, int W, int Cin, int Cout,
            int Cout_pad, const half_t* zero_page, hipStream_t s, float* gn_part /*H W / 256 chunks per image*/, int res_up, int slabs, float* ws, size_t ws_floats);

// ---- the route of ONE conv (nn_gemm.hip): which of the six kernels runs it, with what split, what it leaves behind and what it absorbs.
// conv_plan() is the only place a kernel is chosen; conv_launch() is the only place one is started.  Planning is pure host code and a function
// of its arguments (the hooks come in as a Tuning); the launchers execute the plan: they recompute nothing and read no hook.
enum ConvKernel { CONV_HALO, CONV_RR, CONV_HT, CONV_SK, CONV_IGEMM, CONV_UP_PHASE };
const char* conv_kernel_name(ConvKernel k);
struct ConvNeeds {                 // two_source is a fact of the input; the rest are wishes -- the plan's takes_* say which the kernel absorbs
    bool two_source = false;       //   input = never-materialised channel concat (1x1 only)
    bool in_up = false;            //   input = half-resolution tensor read as its nearest x2
    bool apply = false;            //   GroupNorm (+ FiLM) + SiLU from an (A, B) table while staging (halo kernel)
    bool in_gn = false;            //   the same from the producers' octet partials while staging (row-resident kernel)
    bool want_gn = false;          //   leave GroupNorm octet partials of the output
    int skip_cs = 0;               //   channels of the ResBlock's skip 1x1 to append to the K loop (0 = none)
    bool have_wf = false, have_wf_skip = false;   // fragment-major weights exist (plain / with the skip appended)
};
struct ConvPlan {
    int N = 0, H = 0, W = 0, Cin = 0, Cout = 0, Cout_pad = 0, taps = 0;   // H, W: the resolution the conv runs at (its output's)
    ConvKernel kernel = CONV_IGEMM;
    SkPlan sk{0, 0, 0, 0}; RrPlan rr{0, 0, 0, 0, 0, 0, 0};
    int splits = 1;                // HALO / IGEMM: split-K factor
    bool halo_rows = false;        // HALO, W = 256: tiles of 2 full rows, not 4 x 128 column strips (conv3x3_halo_rows)
    int slabs = 1;                 // HT: K-slabs
    int bk = 0, geo = 0;           // IGEMM: K-step and tile geometry (UP_PHASE: geo)
    int stages = 0;                // IGEMM: LDS stages 2 / 3 / 4, or 12 = two stages + the register-pipelined schedule
    bool want_gn = false;          // the caller keeps room for the output's octet partials
    int gn_chunks = 0;             // octet-partial chunks per image the launch leaves (0 = none): the one place this is computed
    bool takes_res_up = false;     // can read its residual from the half-resolution tensor
    bool takes_in_up = false, takes_apply = false, takes_in_gn = false, takes_skip = false;   // the wishes of ConvNeeds it absorbs
    int skip_cs = 0;               // takes_skip: channels of the appended skip 1x1
};
ConvPlan conv_plan(const Tuning& t, int N, int H, int W, int Cin, int Cout, int Cout_pad, int taps, const ConvNeeds& needs, size_t ws_floats);
// the up-ResBlock phase conv is chosen by the engine (nn_unet.hip), not by precedence; (H, W) = the output, twice the input it reads
ConvPlan conv_up2_phase_plan(const Tuning& t, int N, int H, int W, int Cin, int Cout, int Cout_pad, bool want_gn);
struct ConvArgs {
    const half_t* X; const half_t* X2; int Cin1;      // X2 / Cin1: second tensor of a two-source input
    const half_t* Wt;                                  // the weights in the chosen kernel's layout
    const float* bias; const half_t* residual; int res_up;
    const float* apply_table;                          // takes_apply
    const RrIn* rr_in;                                 // takes_in_gn: the source with its GroupNorm description
    const half_t* XS; const half_t* XS2; int Cs1;      // takes_skip: the skip source [XS (Cs1 channels) | XS2]
    half_t* Y; const half_t* zero_page; float* ws; size_t ws_floats;
    float* gn_part;                                    // room for p.gn_chunks chunks per image (handed to the kernel only when p.gn_chunks > 0)
};
int conv_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t s);

// ---- the GroupNorm (+ FiLM) (+ SiLU) element map (nn_norm.hip's k_gn_apply and nn_conv_rr.hip's staging: ONE definition, bit-identical results)
// x * sigmoid(x); v_rcp_f32 (1 ulp) instead of the IEEE divide sequence: the result is rounded to f16 (or feeds the f32 head,
// tolerance 1e-3) and the divide was half of this HBM-bound kernel's VALU work
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// One element of GroupNorm (+ FiLM) (+ SiLU) with the reference's f16 tensor between the ops.  Every f32 result is made opaque
// before it is rounded to f16: left alone, the compiler fuses an op with the conversion behind it (v_fma_mixlo_f16: ONE rounding) in
// some copies of the loop and not in others -- the 4-pixel main loop and the 1-pixel tail of k_gn_apply differed by one f16 ulp in
// 4e-5 of the elements, so a result depended on the pixels-per-thread a launch happened to pick.
__device__ __forceinline__ float gn_round_f16(float f) { asm("" : "+v"(f)); return (float)(half_t)f; }
template <bool OUT_F32, bool FILM>
__device__ __forceinline__ float gn_elem(float x, float ga, float gb, float t1, float sh, int silu) {
    float f = __builtin_fmaf(x, ga, gb);
    if (!OUT_F32) f = gn_round_f16(f);                                   // GroupNorm32 returns x.dtype (f16)
    if (FILM) {
        f = gn_round_f16(f * t1);
        f = gn_round_f16(f + sh);
    }
    if (silu) { f = silu_f(f); if (!OUT_F32) f = gn_round_f16(f); }
    return f;
}


// ---- normalisation / elementwise (nn_norm.hip)
// GroupNorm(32) statistics of X [N,HW,C] f16 -> stats [N][32][2] (mean, rstd) f32.  ws: N*chunks*32*2 floats.
int gn_stats(const half_t* X, int N, int HW, int C, float eps, float* stats, float* ws, size_t ws_floats, hipStream_t s);
// y = silu?( GN(x)*gamma+beta [*(1+scale)+shift] ), optional 2x resample; RESAMPLE: 0 none, 1 avgpool2, 2 nearest-up2.
// film: rows of (scale[C] | shift[C]) f32, row n at film + n*film_stride, or null.  Output f16 NHWC (or f32 when out_f32).
// parts != NULL (stats == NULL): the statistics are reduced inside the apply kernel from the producing convs' octet partials
// (what gn_finalize_oct would read) -- the small-batch form, one launch less per GroupNorm
struct GnPartsArg { const float* partA; int Ca, chunksA; const float* partB; int Cb, chunksB; float eps; };
int gn_apply(const half_t* X, const float* stats, const float* gamma, const float* beta, const float* film,
             long long film_stride, int N, int H, int W, int C, int silu, int resample, void* Y, int out_f32, hipStream_t s,
             const half_t* XB = nullptr, int Ca = 0,      // XB: second tensor of a never-materialised channel concat
             half_t* Yraw = nullptr,                      // resample 1 only: also AvgPool2d(2) of the RAW input (the x branch of a down-ResBlock)
             const GnPartsArg* parts = nullptr,
             int iters_hook = 0);                         // Tuning::gn_iters
// GroupNorm (+ FiLM) as one affine map per (image, channel): table [N][C/8][16] = (A0..A7, B0..B7) per channel octet, y = silu(A x + B) -- the
// input transform of the APPLY variant of the halo conv (the stand-alone gn_apply pass disappears)
int gn_table(const float* stats, const float* gamma, const float* beta, const float* film, long long film_stride, int N, int C,
             float* table, hipStream_t s);
// GroupNorm-apply (+ SiLU) of a ResBlock input AND the block's skip 1x1 conv (C -> 256) in one pass over x = [XA | XB] (channel concat,
// XB may be null when Ca == C): H0 [N,HW,C] = silu(GN(x)), SK [N,HW,256] = f16(Wt x + bias).  stats [N][32][2] finished.
bool gn_skip_eligible(int N, int HW, int Ca, int C, int Cout, int Cout_pad);
int gn_skip(const half_t* XA, const half_t* XB, int Ca, int C, const float* stats, const float* gamma, const float* beta, const half_t* Wt,
            const float* bias, half_t* H0, half_t* SK, int N, int HW, hipStream_t s, int variant /*Tuning::gs_variant*/);
int resample2x(const half_t* X, int N, int H, int W, int C, int mode, half_t* Y, hipStream_t s);
int concat_channels(const half_t* A, int Ca, const half_t* B, int Cb, long long pixels, half_t* Y, hipStream_t s);

// ---- attention (nn_attn.hip): QKVAttentionLegacy on qkv [N,T,3C] f16 (per head h: q|k|v at channel h*3*D), out [N,T,C].
// vt_ws: N*T*C halfs (transposed V); nbuf / qtn / vt: Tuning::attn_*
int attention(const half_t* qkv, half_t* out, int N, int T, int C, int D, hipStream_t s, half_t* vt_ws, int nbuf, int qtn, int vt);

// ---- small dense ops (nn_misc.hip)
// p: the plan of the 1x1 conv over the im2col rows (conv_plan(t, N, H, W, 32, Cout, Cout_pad, 1, needs, 0)); gn_part: room for p.gn_chunks chunks per image
int conv_in_3x3(const ConvPlan& p, const float* x_nchw, const half_t* Wt /*[Cout_pad][32] k=(ky*3+kx)*3+c, k>=27 zero*/, const float* bias, half_t* Y,
                int N, int H, int W, int Cout, int Cout_pad, half_t* im2col_ws /*[N*H*W][32]*/, const half_t* zero_page, hipStream_t s, float* gn_part = nullptr);
// output head (nn_head.hip): GroupNorm affine -> SiLU -> conv3x3 (C -> 3|6) in f32-equivalent arithmetic, y f32 NCHW.
// wz = head_pack(w f32 [NO][9*C] (k = tap*C + c)): [2][64][C] f16 hi/lo.
int head_pack(const float* w, int NO, int C, half_t* wz, hipStream_t s);
int head_gn_silu_conv3x3(const half_t* X, const float* stats, const float* gamma, const float* beta, const half_t* wz,
                         const float* bias, float* y_nchw, int N, int H, int W, int C, int NO, hipStream_t s);
int timestep_mlp(const float* t, int N, int mc, const float* w0, const float* b0, const float* w2, const float* b2,
                 float* emb_silu /*[N][4mc] = silu(time_embed(t))*/, float* tmp, hipStream_t s);
int gemv_rows(const float* Wm /*[R][K]*/, const float* b, const float* x /*[N][K]*/, float* y /*[N][R]*/, int R, int K, int N,
              hipStream_t s);

// ---- DDNM (nn_misc.hip)
struct DdnmCoef { float sqrt_1m_at, sqrt_at, sqrt_at_next, sigma_t, c1, c2; };
int ddnm_update(float* x /*[N,3,HW] in/out*/, const float* et /*[N,Cet,HW], first 3 used*/, int Cet, const float* y,
                const float* mask /*[N,HW]*/, const float* eps /*null -> philox*/, unsigned long long seed,
                unsigned long long step, DdnmCoef co, int N, int HW, hipStream_t s, unsigned long long quad0 = 0);
int ddnm_prepare(const float* masked_img, const float* mask, float* y, int N, int HW, hipStream_t s);
int ddnm_finish(const float* x, float* out, long long n, hipStream_t s);
// Philox counter = (quad0 + element / 4, stream_id), key = seed.  quad0 = first image key * quads per image makes the noise of an
// image a function of its KEY only (not of its position in the batch or of how views are sharded over ranks).
int copy16(const void* src, void* dst, long long bytes, int blocks, int unroll, hipStream_t s);   // calibration copy (nn_misc.hip)
int philox_normal(float* out, long long n, unsigned long long seed, unsigned long long stream_id, hipStream_t s,
                  unsigned long long quad0 = 0);

}  // namespace pdnn
