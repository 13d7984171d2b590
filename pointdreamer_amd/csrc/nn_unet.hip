// Rows U1 + D1: the guided-diffusion UNet engine and the DDNM sampler behind the C ABI.
// Graph construction mirrors UNetModel.__init__ (models/DDNM/guided_diffusion/unet.py:481-617) as configured
// by script_util.create_model (:130-185); weights are loaded under the reference's state-dict names
// (`input_blocks.N.M.in_layers.2.weight`, ...) and repacked on the device into the kernels' layouts:
//   conv3x3 / conv1x1 / conv1d(k=1) weights -> f16 [Cout_pad][taps*Cin] (k = tap*Cin + c), biases f16-rounded f32,
//   time_embed / emb_layers Linear and all GroupNorm affine and the `out` head stay f32 (fp16_util.py:15-22).
// Activations are NHWC f16 in a bump arena sized at create() for max_batch (288 GB HBM: no reuse games);
// every forward issues the same launches at the same addresses, asynchronously on the caller's stream.
#include "nn_common.h"
#include "nn_conv_tail.h"
#include <map>
#include <string>
#include <vector>
#include <cmath>
#include <cstring>
using namespace pdhip;
using namespace pdnn;

namespace {

struct ConvW { half_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, cout_pad = 0, taps = 0; bool have_w = false, have_b = false;
               half_t* wf = nullptr; half_t* wph = nullptr; bool has_wf = false, has_wph = false; };   // has_*: fixed at graph build, what routing asks; allocation follows them   // wf: fragment-major copy for the row-resident kernel (nn_conv_rr.hip), the 3x3 convs of the <= 64^2 levels; packed at load time   // wph: phase weights [4][cout_pad][4 cin] of an up-ResBlock's in_layers conv (conv_up2_phase), packed at load time
struct NormW { float* g = nullptr; float* b = nullptr; int c = 0; bool have_g = false, have_b = false; };
struct ResB { std::string name; int cin, cout, mode; NormW n1, n2; ConvW c1, c2, skip; long long emb_off; bool has_skip; bool have_ew = false, have_eb = false;
              half_t* c2s_w = nullptr; float* c2s_b = nullptr; bool c2s_ready = false; half_t* c2s_wf = nullptr; int hw = 0; bool has_c2s = false, has_c2s_wf = false; };   // hw: resolution the block's convs run at   // conv2 with the skip 1x1 appended to its K loop (conv_sk_skip), built by pdhip_unet_load_tensor once its four sources are loaded
struct AttB { std::string name; int c; NormW n; ConvW qkv, proj; };
struct Block { int kind; int idx; };          // 0 conv_in, 1 res, 2 attn

// gn_part: octet partial sums fused into the producing conv's epilogue ([N][chunks][C/8][2]); for a channel concat the
// second source's partials are gn_partB (first Ca channels come from gn_part)
struct Act { half_t* p; int C, H, W; const float* gn_part = nullptr; int gn_chunks = 0; const float* gn_partB = nullptr; int Ca = 0; int gn_chunksB = 0;
             half_t* p2 = nullptr;      // p2: virtual channel concat [p (Ca channels) | p2 (C - Ca channels)], never materialised
             int row = -1, rowB = -1; };   // route table only: the rows of the convs that produced p / p2

}  // namespace
namespace pdnn {
Tuning& tuning() { static thread_local Tuning t; return t; }
}
// the stand-alone conv entry's split-K workspace (pdhip_debug_set_conv_splitk): state, not tuning -- read by the C entry points below only
static thread_local float* g_dbg_splitk_ws = nullptr;
static thread_local size_t g_dbg_splitk_floats = 0;
namespace {
struct Prof { std::vector<hipEvent_t> ev; std::vector<uint8_t> cls; size_t used = 0; double flops[2] = {0, 0}; bool on = false;
              int period = 1; long long forwards = 0; bool armed = false; };   // cls 0: halo 3x3 conv, 1: attention

}  // namespace

struct pdhip_unet {
    int image_size, mc, nres, head, out_ch, max_batch, ted;
    std::vector<int> mult, att_ds;
    std::vector<ResB> res;
    std::vector<AttB> att;
    std::vector<std::vector<Block>> input, output;
    std::vector<Block> middle;
    int final_ch;
    // parameters
    half_t* w_in = nullptr; float* b_in = nullptr; bool have_win = false, have_bin = false;
    float *te_w0 = nullptr, *te_b0 = nullptr, *te_w2 = nullptr, *te_b2 = nullptr; bool have_te[4] = {false, false, false, false};
    float *emb_w = nullptr, *emb_b = nullptr; long long emb_rows = 0;
    NormW out_norm; float* out_w = nullptr; float* out_b = nullptr; bool have_ow = false, have_ob = false;
    half_t* zero_page = nullptr;
    // workspace
    char* arena = nullptr; size_t arena_bytes = 0, arena_off = 0; bool arena_overflow = false;
    float *stats = nullptr, *gn_ws = nullptr; size_t gn_ws_floats = 0;
    float* ap_table = nullptr;                   // GroupNorm (+ FiLM) folded to (A, B) per (image, channel) for the conv that applies it while staging
    float *emb_silu = nullptr, *emb_tmp = nullptr, *emb_all = nullptr;
    // DDNM sampler: the embeddings of all (<= 100) schedule steps, computed in ONE pass over the 180 MB of emb_layers weights
    // and kept until the weights change (every image of a sampling step shares t, so the per-step forward reads one row)
    float *steps_t = nullptr, *steps_silu = nullptr, *steps_tmp = nullptr, *steps_emb = nullptr; int steps_cached = 0;
    half_t* head_wz = nullptr;                   // output-head weights as f16 hi/lo pairs (nn_head.hip)
    half_t* head_wz3 = nullptr;                  // the same for output channels 0..2 only: the DDNM sampler discards the variance
                                                 // channels of a learn_sigma net (diffusion.py:527-528: et = et[:, :3]) -- half the head
    float *t_dev = nullptr;
    float* splitk_ws = nullptr; size_t splitk_floats = 0;
    // sampler state
    float *sx = nullptr, *sy = nullptr, *set_ = nullptr, *smask = nullptr;
    Prof prof;
    std::vector<void*> owned;
};

namespace {

template <typename T>
int dalloc(pdhip_unet* u, T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 256));
    if (e != hipSuccess) { set_error("hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e)); return PDHIP_E_NOMEM; }
    u->owned.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return PDHIP_OK;
}
#define PD_TRY(expr) do { int rc_ = (expr); if (rc_ != PDHIP_OK) return rc_; } while (0)

int alloc_conv(pdhip_unet* u, ConvW& c) {      // (shape: build_graph)
    PD_TRY(dalloc(u, &c.w, (size_t)c.cout_pad * c.taps * c.cin));
    PD_HIP(hipMemset(c.w, 0, (size_t)c.cout_pad * c.taps * c.cin * sizeof(half_t)));
    PD_TRY(dalloc(u, &c.b, (size_t)c.cout));
    return PDHIP_OK;
}
int alloc_norm(pdhip_unet* u, NormW& n, int c) {
    n.c = c;
    PD_TRY(dalloc(u, &n.g, (size_t)c));
    PD_TRY(dalloc(u, &n.b, (size_t)c));
    return PDHIP_OK;
}

// ---- weight repack kernels
__global__ void k_pack_conv(const void* __restrict__ src, int src_f16, int Cout, int Cin, int taps, half_t* __restrict__ dst) {
    // src [Cout][Cin][taps] (PyTorch OIHW flattened) -> dst [Cout][taps*Cin], k = tap*Cin + c
    const long long total = (long long)Cout * Cin * taps;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        const int c = (int)((i / taps) % Cin);
        const int o = (int)(i / ((long long)taps * Cin));
        const float v = src_f16 ? (float)reinterpret_cast<const half_t*>(src)[i] : reinterpret_cast<const float*>(src)[i];
        dst[(size_t)o * taps * Cin + (size_t)tap * Cin + c] = (half_t)v;
    }
}
__global__ void k_pack_conv_in(const void* __restrict__ src, int src_f16, int Cout, half_t* __restrict__ dst) {
    // src [Cout][3][3][3] (OIHW) -> dst [Cout][32], k = (ky*3+kx)*3 + c  (columns 27..31 stay zero)
    const int total = Cout * 27;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int tap = i % 9, c = (i / 9) % 3, o = i / 27;
        const float v = src_f16 ? (float)reinterpret_cast<const half_t*>(src)[i] : reinterpret_cast<const float*>(src)[i];
        dst[(size_t)o * 32 + tap * 3 + c] = (half_t)v;
    }
}
__global__ void k_pack_conv_f32(const void* __restrict__ src, int src_f16, int Cout, int Cin, int taps, float* __restrict__ dst) {
    const long long total = (long long)Cout * Cin * taps;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        const int c = (int)((i / taps) % Cin);
        const int o = (int)(i / ((long long)taps * Cin));
        const float v = src_f16 ? (float)reinterpret_cast<const half_t*>(src)[i] : reinterpret_cast<const float*>(src)[i];
        dst[(size_t)o * taps * Cin + (size_t)tap * Cin + c] = v;
    }
}
__global__ void k_copy_f32(const void* __restrict__ src, int src_f16, long long n, float* __restrict__ dst, int round_f16) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = src_f16 ? (float)reinterpret_cast<const half_t*>(src)[i] : reinterpret_cast<const float*>(src)[i];
        if (round_f16) v = (float)(half_t)v;
        dst[i] = v;
    }
}
int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 4096); }

// ---- arena
half_t* arena_take(pdhip_unet* u, size_t halfs) {
    size_t bytes = (halfs * sizeof(half_t) + 255) & ~(size_t)255;
    if (u->arena == nullptr) { u->arena_off += bytes; return nullptr; }      // dry run (sizing)
    if (u->arena_off + bytes > u->arena_bytes) { u->arena_overflow = true; return reinterpret_cast<half_t*>(u->arena); }   // (reported by forward_impl)
    half_t* p = reinterpret_cast<half_t*>(u->arena + u->arena_off);
    u->arena_off += bytes;
    return p;
}

struct Act;
struct Table { std::vector<std::string> name, line; };      // pdhip_unet_route_table: one line per conv of a forward
struct Ctx { pdhip_unet* u; int N; hipStream_t s; bool dry; const float* film_base; long long film_stride; Table* table;
             Tuning t;      // the hooks this forward is planned and run under (taken once by the entry point)
             bool go() const { return !dry && table == nullptr; } };   // go: a real forward; dry: the sizing pass; table: planning only (real routing, no launches)

int prof_begin(Ctx& c, double flops, int cls = 0) {
    Prof& p = c.u->prof;
    if (!p.on || !p.armed || !c.go()) return PDHIP_OK;
    if (p.used + 2 > p.ev.size()) {
        for (int i = 0; i < 256; ++i) { hipEvent_t e; PD_HIP(hipEventCreate(&e)); p.ev.push_back(e); p.cls.push_back(0); }
    }
    PD_HIP(hipEventRecord(p.ev[p.used], c.s));
    p.cls[p.used] = (uint8_t)cls;
    p.flops[cls] += flops;
    return PDHIP_OK;
}
int prof_end(Ctx& c) {
    Prof& p = c.u->prof;
    if (!p.on || !p.armed || !c.go()) return PDHIP_OK;
    PD_HIP(hipEventRecord(p.ev[p.used + 1], c.s));
    p.used += 2;
    return PDHIP_OK;
}

// room for a conv's octet partials: [N][chunks][cout/8][2] floats, chunks <= HW/16 (split-K reduce) -- sized for the finest chunking
float* take_parts(Ctx& c, int H, int W, int cout) {
    return reinterpret_cast<float*>(arena_take(c.u, (size_t)c.N * ((H * W + 15) / 16) * (cout / 8) * 2 * 2));
}
void adopt_parts(Act* out, float* part, int chunks) {
    if (part != nullptr && chunks > 0) { out->gn_part = part; out->gn_chunks = chunks; out->Ca = out->C; }
}

// what a conv reads besides its plan: x (raw when the plan absorbs the GroupNorm), the residual, and the sources of what the plan absorbs
struct ConvIn { const Act* x; const half_t* residual = nullptr; int res_up = 0; const float* apply_table = nullptr; const RrIn* rr_in = nullptr;
                const Act* skip_src = nullptr; const ResB* skip_w = nullptr;      // takes_skip: the block input and the block holding the fused weights
                const Act* parts_of = nullptr; const char* note = nullptr; };     // route table only: the tensor whose partials this conv's input pass depends on

void table_row(Ctx& c, const std::string& name, const ConvPlan& p, const ConvIn& in, Act* out) {
    char detail[64];
    switch (p.kernel) {
    case CONV_HALO: case CONV_IGEMM: snprintf(detail, sizeof detail, "splits=%d", p.splits); break;
    case CONV_HT: snprintf(detail, sizeof detail, "slabs=%d", p.slabs); break;
    case CONV_RR: snprintf(detail, sizeof detail, "variant=%d,slabs=%d", p.rr.variant, p.rr.S0); break;
    case CONV_SK: snprintf(detail, sizeof detail, "tile=%dx%d,splits=%d", p.sk.bm, p.sk.bn, p.sk.splits); break;
    default: snprintf(detail, sizeof detail, "-"); break;
    }
    std::string folds;
    auto add = [&](const std::string& f) { folds += (folds.empty() ? "" : ",") + f; };
    if (in.note) add(in.note);
    if (in.x->p2) add("two_source");
    if (p.takes_apply) add("apply");
    if (p.takes_in_gn) add("in_gn");
    if (p.takes_in_up) add("in_up");
    if (in.res_up) add("res_up");
    if (p.takes_skip) add("skip");
    if (in.parts_of) {
        const Act& a = *in.parts_of;
        add("parts<-" + (a.gn_part && a.row >= 0 ? c.table->name[a.row] : std::string("?")) +
            (a.p2 ? "+" + (a.gn_partB && a.rowB >= 0 ? c.table->name[a.rowB] : std::string("?")) : std::string()));
    }
    char line[512];
    snprintf(line, sizeof line, "%s %dx%d %d->%d %s %s gn=%d %s", name.c_str(), p.H, p.W, p.Cin, p.Cout, conv_kernel_name(p.kernel), detail, p.gn_chunks,
             folds.empty() ? "-" : folds.c_str());
    out->row = (int)c.table->line.size();
    c.table->name.push_back(name);
    c.table->line.push_back(line);
}

// one conv, as planned: output (+ partials) from the arena, then the launch
int run_conv(Ctx& c, const std::string& name, const ConvPlan& p, const ConvW& w, const ConvIn& in, Act* out) {
    *out = Act{nullptr, p.Cout, p.H, p.W};
    out->p = arena_take(c.u, (size_t)c.N * p.H * p.W * p.Cout);
    float* part = p.want_gn ? take_parts(c, p.H, p.W, p.Cout) : nullptr;
    if (c.table) table_row(c, name, p, in, out);
    if (!c.dry) adopt_parts(out, part, p.gn_chunks);
    if (!c.go()) return PDHIP_OK;
    PD_REQUIRE(w.have_w && w.have_b, "unet: weights of %s not loaded", name.c_str());
    const ResB* fs = p.takes_skip ? in.skip_w : nullptr;
    PD_REQUIRE(fs == nullptr || (fs->skip.have_w && fs->skip.have_b && fs->c2s_ready), "unet: fused conv2 + skip weights of %s were not built at load time", name.c_str());
    const half_t* wt = fs ? (p.kernel == CONV_RR ? fs->c2s_wf : fs->c2s_w) : p.kernel == CONV_RR ? w.wf : p.kernel == CONV_UP_PHASE ? w.wph : w.w;
    const Act& x = *in.x;
    const Act* xs = p.takes_skip ? in.skip_src : nullptr;
    const ConvArgs a{x.p, x.p2, x.p2 ? x.Ca : 0, wt, fs ? fs->c2s_b : w.b, in.residual, in.res_up, in.apply_table, in.rr_in,
                     xs ? xs->p : nullptr, xs ? xs->p2 : nullptr, xs && xs->p2 ? xs->Ca : 0, out->p, c.u->zero_page, c.u->splitk_ws, c.u->splitk_floats, part};
    // profile hook (bench.py roofline): the dominant kernel only -- the halo-resident 3x3 conv, unsplit
    const bool booked = p.kernel == CONV_HALO && p.splits == 1;
    if (booked) PD_TRY(prof_begin(c, 2.0 * c.N * p.H * p.W * (double)p.Cout * 9.0 * p.Cin));
    PD_TRY(conv_launch(p, a, c.s));
    return booked ? prof_end(c) : PDHIP_OK;
}
ConvPlan plan_conv(const Ctx& c, const Act& x, const ConvW& w, bool want_gn) {      // a conv outside the ResBlocks: nothing to absorb
    ConvNeeds nd;
    nd.two_source = x.p2 != nullptr; nd.want_gn = want_gn; nd.have_wf = w.has_wf;
    return conv_plan(c.t, c.N, x.H, x.W, w.cin, w.cout, w.cout_pad, w.taps, nd, c.u->splitk_floats);
}

// GroupNorm statistics of x: from the fused conv-epilogue partials when available, else a pass over the tensor
int run_gn_stats(Ctx& c, const Act& x) {
    if (x.gn_part != nullptr && ((x.C / 32) % 8) == 0)
        return gn_finalize_oct(x.gn_part, x.Ca, x.gn_chunks, x.gn_partB, x.C - x.Ca, x.gn_chunksB, c.N, x.H * x.W, 1e-5f, c.u->stats, c.s);
    PD_REQUIRE(x.p2 == nullptr, "unet: a virtual concat needs fused GroupNorm partials of both tensors");
    return gn_stats(x.p, c.N, x.H * x.W, x.C, 1e-5f, c.u->stats, c.u->gn_ws, c.u->gn_ws_floats, c.s);
}

int run_gn(Ctx& c, const Act& x, const NormW& n, const float* film, long long film_stride, int silu, int resample, Act* out,
           half_t* raw_pool = nullptr) {
    *out = Act{nullptr, x.C, 0, 0};
    out->H = resample == 1 ? x.H / 2 : (resample == 2 ? x.H * 2 : x.H);
    out->W = resample == 1 ? x.W / 2 : (resample == 2 ? x.W * 2 : x.W);
    out->p = arena_take(c.u, (size_t)c.N * out->H * out->W * x.C);
    if (!c.go()) return PDHIP_OK;
    PD_REQUIRE(n.have_g && n.have_b, "unet: norm weights not loaded");
#ifdef PD_LAB_SKIP_GN                                       // (lab, timing only -- WRONG results: what the small-level GroupNorm-apply launches cost)
    if (resample == 0 && x.p2 == nullptr && x.W <= 128 && silu) { out->p = x.p; return PDHIP_OK; }
#endif
    // small batches: the apply kernel reduces the octet partials itself (no k_gn_finalize_oct launch); large batches: every
    // workgroup re-reducing its image's partials costs more than the 5 us launch it removes
    if (x.gn_part != nullptr && ((x.C / 32) % 8) == 0 && (x.C >> 3) <= 256 && c.t.fold_finalize > 0 &&
        (c.N <= c.t.fold_finalize || (x.gn_chunks <= c.t.fold_finalize_chunks && x.gn_chunksB <= c.t.fold_finalize_chunks))) {
        const GnPartsArg pa{x.gn_part, x.Ca, x.gn_chunks, x.gn_partB, x.C - x.Ca, x.gn_chunksB, 1e-5f};
        return gn_apply(x.p, nullptr, n.g, n.b, film, film_stride, c.N, x.H, x.W, x.C, silu, resample, out->p, 0, c.s, x.p2,
                        x.p2 ? x.Ca : 0, raw_pool, &pa, c.t.gn_iters);
    }
    PD_TRY(run_gn_stats(c, x));
    return gn_apply(x.p, c.u->stats, n.g, n.b, film, film_stride, c.N, x.H, x.W, x.C, silu, resample, out->p, 0, c.s, x.p2, x.p2 ? x.Ca : 0,
                    raw_pool, nullptr, c.t.gn_iters);
}

// GroupNorm (+ FiLM) + SiLU of x, then the conv, in the form the plan took:
//   takes_apply  statistics -> (A, B) table -> the halo-resident kernel transforms its input tile of the RAW tensor in LDS (nn_conv_halo.hip APPLY)
//   takes_in_gn  the row-resident kernel normalises the RAW tensor while staging, from the producer's octet partials (nn_conv_rr.hip; see Tuning::rr_gn)
//   neither      a stand-alone GroupNorm-apply pass (with the block's resampling, and AvgPool2d(2) of the raw input into raw_pool), then the conv
// In the first two the stand-alone pass and its output tensor disappear; all three give the same bits.
int run_gn_then_conv(Ctx& c, const std::string& name, const ConvPlan& p, const Act& x, const NormW& n, const float* film, long long film_stride,
                     int resample, half_t* raw_pool, const ConvW& w, ConvIn in, Act* out) {
    if (p.takes_apply) {
        if (c.go()) {
            PD_REQUIRE(n.have_g && n.have_b, "unet: norm weights not loaded");
            PD_TRY(run_gn_stats(c, x));
            PD_TRY(gn_table(c.u->stats, n.g, n.b, film, film_stride, c.N, x.C, c.u->ap_table, c.s));
            in.apply_table = c.u->ap_table;
        }
        in.x = &x;
        return run_conv(c, name, p, w, in, out);
    }
    if (p.takes_in_gn) {
        if (c.go()) PD_REQUIRE(n.have_g && n.have_b, "unet: norm weights not loaded");
        const RrIn rr_in{x.p, nullptr, x.C, x.C, 2, n.g, n.b, film, film_stride, x.gn_part, nullptr, x.gn_chunks, 0, 1e-5f};
        in.x = &x; in.rr_in = &rr_in; in.parts_of = &x;
        return run_conv(c, name, p, w, in, out);
    }
    Act h;
    PD_TRY(run_gn(c, x, n, film, film_stride, 1, resample, &h, raw_pool));
    in.x = &h;
    if (x.p2 != nullptr) in.parts_of = &x;
    return run_conv(c, name, p, w, in, out);
}

// ---- the plan of one ResBlock: pure host code, decided before anything is taken from the arena or launched
struct ResPlan {
    bool fuse_skip = false;        // in_layers' GroupNorm-apply and the skip 1x1 read the same (virtual concat) input: one pass (k_gn_skip)
    bool fold_down = false;        // x branch of a down block: AvgPool2d(2)(x) is the second output of the GroupNorm-apply pass
    bool fold_up = false;          // x branch of an up block: nearest x2 is index arithmetic in conv2's residual read (c2.takes_res_up)
    bool skip_conv = false;        // the skip 1x1 runs as a launch of its own (plan: skip)
    ConvPlan c1, c2, skip;         // c1: takes_apply / takes_in_gn / CONV_UP_PHASE / takes_in_up say its form; c2: takes_skip / takes_apply / takes_in_gn
};
// the row-resident kernel's in-staging GroupNorm is wished for where it measured a gain (t.rr_gn) and the input carries what it reads
bool wish_in_gn(const Tuning& t, const Act& x, const ConvW& w, int W) {
    if (t.rr_gn <= 0 || W > t.rr_gn || x.p2 != nullptr || x.gn_part == nullptr || x.gn_partB != nullptr || ((x.C / 32) % 8) != 0 || w.cin > 1024 ||
        x.C != w.cin) return false;
    const int cs = conv_rr_gn_unit(t, W);                // a unit of the variant the plan would take must fit that variant's statistics tables
    if (cs == 0 || rr_gn_groups_max(cs, x.C) > rr_gn_groups_cap(cs)) return false;
    const int pps = std::max(1, 256 / (x.C >> 3));
    return (x.gn_chunks + pps - 1) / pps <= PD_RR_MAX_PART_LOADS;
}
// the up-ResBlock in_layers conv on the phase kernel?  (H, W: the half-resolution input)
bool wish_up_phase(const Tuning& t, int N, const ResB& rb, int H, int W) {
    if (t.up_phase == 0 || rb.mode != 2 || !rb.c1.has_wph || (H * W) % 256 != 0 ||
        !conv_up2_phase_eligible(N, H, W, rb.c1.cin, rb.c1.cout, rb.c1.cout_pad)) return false;
    if (t.up_phase == 2) return true;
    // automatic, by measurement (profiles/up_phase_layers.txt, batch 1 ... 32 x the five up blocks): from 128 tiles (4 phases x 256-pixel tiles x
    // channel tiles) on the phase conv beat the 9-tap route in every case (1.19x at 128 tiles ... 1.94x), at 64 tiles and below it lost (0.23 ... 0.92x:
    // 256 x 256 tiles on a quarter of the CUs)
    const long long tiles = (long long)N * H * W / 256 * 4 * (rb.c1.cout_pad / (rb.c1.cout_pad % 256 == 0 ? 256 : 128));
    return tiles >= 128;
}
// conservative = the sizing pass: every tensor a routing could need is materialised (two-pass GroupNorm, resampled x branch, skip tensor), since
// the hooks and the batch of a later forward may route differently; it assumes the input carries partials (k_gn_skip's two outputs are the larger form)
ResPlan plan_res(const Tuning& t, int N, size_t ws_floats, bool conservative, const Act& x, const ResB& rb) {
    ResPlan r;
    const int Ho = rb.mode == 1 ? x.H / 2 : (rb.mode == 2 ? x.H * 2 : x.H), Wo = rb.mode == 1 ? x.W / 2 : (rb.mode == 2 ? x.W * 2 : x.W);
    const bool lean = !conservative;
    // x branch of an up / down block (unet.py:190-195, 237-242: h and x go through the same Upsample / Downsample)
    const bool fold = t.fold_resample != 0 && lean && x.p2 == nullptr && !rb.has_skip;
    r.fold_down = fold && rb.mode == 1;
    r.fuse_skip = rb.has_skip && rb.mode == 0 && t.fuse_skip != 0 && rb.skip.taps == 1 && x.C == rb.skip.cin &&
                  gn_skip_eligible(N, x.H * x.W, x.p2 ? x.Ca : x.C, x.C, rb.skip.cout, rb.skip.cout_pad) &&
                  (t.fuse_skip == 2 || (long long)N * x.H * x.W / 128 >= t.fuse_skip_min_tiles) &&
                  (conservative || (x.gn_part != nullptr && ((x.C / 32) % 8) == 0));
    ConvNeeds n1;
    n1.want_gn = true; n1.have_wf = rb.c1.has_wf;
    if (lean && !r.fuse_skip && rb.mode == 0 && x.p2 == nullptr) { n1.apply = t.fuse_gn != 0; n1.in_gn = wish_in_gn(t, x, rb.c1, x.W); }
    n1.in_up = fold && rb.mode == 2;       // nearest x2 of the normalised input: index arithmetic in conv1's halo staging, the GroupNorm pass stays at half resolution
    if (lean && x.p2 == nullptr && !rb.has_skip && wish_up_phase(t, N, rb, x.H, x.W))
        r.c1 = conv_up2_phase_plan(t, N, Ho, Wo, rb.c1.cin, rb.c1.cout, rb.c1.cout_pad, true);   // GroupNorm at half resolution, the x2 lives in the weights
    else
        r.c1 = conv_plan(t, N, Ho, Wo, rb.c1.cin, rb.c1.cout, rb.c1.cout_pad, 9, n1, ws_floats);
    // conv2 reads h1 = conv1's output; small-M layers: the skip 1x1 rides in its K loop (no launch of its own, no skip tensor, no residual read)
    Act h1{nullptr, rb.cout, Ho, Wo};
    if (r.c1.gn_chunks > 0) { h1.gn_part = x.gn_part ? x.gn_part : reinterpret_cast<const float*>(&r); h1.gn_chunks = r.c1.gn_chunks; h1.Ca = rb.cout; }
    ConvNeeds n2;
    n2.want_gn = true; n2.have_wf = rb.c2.has_wf;
    if (lean) { n2.apply = t.fuse_gn != 0; n2.in_gn = wish_in_gn(t, h1, rb.c2, Wo); }
    if (lean && rb.has_skip && !r.fuse_skip && t.fold_skip != 0 && rb.mode == 0 && rb.has_c2s && rb.skip.taps == 1 &&
        (x.p2 == nullptr || (x.Ca % 64 == 0 && (x.C - x.Ca) % 64 == 0))) {
        n2.skip_cs = rb.skip.cin;
        n2.have_wf_skip = rb.has_c2s_wf && (x.p2 == nullptr || (x.Ca % 128 == 0 && (x.C - x.Ca) % 128 == 0));
    }
    r.c2 = conv_plan(t, N, Ho, Wo, rb.c2.cin, rb.c2.cout, rb.c2.cout_pad, 9, n2, ws_floats);
    r.fold_up = fold && rb.mode == 2 && r.c2.takes_res_up;
    r.skip_conv = rb.has_skip && !r.fuse_skip && !r.c2.takes_skip;
    if (r.skip_conv) {
        ConvNeeds ns;
        ns.two_source = x.p2 != nullptr;
        r.skip = conv_plan(t, N, Ho, Wo, rb.skip.cin, rb.skip.cout, rb.skip.cout_pad, rb.skip.taps, ns, ws_floats);
    }
    return r;
}

int run_res(Ctx& c, const Act& x, ResB& rb, Act* out) {
    const ResPlan r = plan_res(c.t, c.N, c.u->splitk_floats, c.dry, x, rb);
    Act h1, xr = x, sk;
    const float* film = c.go() ? c.film_base + rb.emb_off : nullptr;
    if (c.go()) PD_REQUIRE(rb.have_ew && rb.have_eb, "unet: emb_layers of %s not loaded", rb.name.c_str());
    if (rb.mode != 0) {
        xr.H = r.c2.H; xr.W = r.c2.W;
        xr.p = arena_take(c.u, (size_t)c.N * xr.H * xr.W * x.C);     // (always reserved: the sizing pass cannot know the folds of a later forward)
    }
    const std::string n1 = rb.name + ".in_layers.2";
    if (r.fuse_skip) {
        Act h0{nullptr, x.C, x.H, x.W};
        h0.p = arena_take(c.u, (size_t)c.N * x.H * x.W * x.C);
        sk = Act{nullptr, rb.skip.cout, x.H, x.W};
        sk.p = arena_take(c.u, (size_t)c.N * x.H * x.W * rb.skip.cout);
        if (c.go()) {
            PD_REQUIRE(rb.n1.have_g && rb.n1.have_b && rb.skip.have_w && rb.skip.have_b, "unet: norm / skip weights of %s not loaded", rb.name.c_str());
            PD_TRY(run_gn_stats(c, x));
            PD_TRY(gn_skip(x.p, x.p2, x.p2 ? x.Ca : x.C, x.C, c.u->stats, rb.n1.g, rb.n1.b, rb.skip.w, rb.skip.b, h0.p, sk.p, c.N, x.H * x.W, c.s, c.t.gs_variant));
        }
        ConvIn in{&h0};
        in.parts_of = &x; in.note = "gn_skip";
        PD_TRY(run_conv(c, n1, r.c1, rb.c1, in, &h1));
    } else {
        const bool half_res = r.c1.kernel == CONV_UP_PHASE || r.c1.takes_in_up;       // the GroupNorm pass stays at the input's resolution
        PD_TRY(run_gn_then_conv(c, n1, r.c1, x, rb.n1, nullptr, 0, half_res ? 0 : rb.mode, r.fold_down ? xr.p : nullptr, rb.c1, ConvIn{nullptr}, &h1));
    }
    if (rb.mode != 0 && c.go() && !r.fold_down && !r.fold_up) PD_TRY(resample2x(x.p, c.N, x.H, x.W, x.C, rb.mode, xr.p, c.s));
    if (!r.fuse_skip) sk = r.fold_up ? x : xr;
    if (r.skip_conv) PD_TRY(run_conv(c, rb.name + ".skip_connection", r.skip, rb.skip, ConvIn{&xr}, &sk));
    ConvIn in2{nullptr, r.c2.takes_skip ? nullptr : sk.p, r.fold_up ? 1 : 0};
    in2.skip_src = &x; in2.skip_w = &rb;
    return run_gn_then_conv(c, rb.name + ".out_layers.3", r.c2, h1, rb.n2, film, c.film_stride, 0, nullptr, rb.c2, in2, out);
}

int run_att(Ctx& c, const Act& x, AttB& ab, Act* out) {
    Act xn, qkv, a;
    PD_TRY(run_gn(c, x, ab.n, nullptr, 0, 0, 0, &xn));
    PD_TRY(run_conv(c, ab.name + ".qkv", plan_conv(c, xn, ab.qkv, false), ab.qkv, ConvIn{&xn}, &qkv));
    a = x;
    a.p = arena_take(c.u, (size_t)c.N * x.H * x.W * x.C);
    half_t* vt = arena_take(c.u, (size_t)c.N * x.H * x.W * x.C);      // transposed V of the T >= 128 attention kernel
    if (c.go()) {
        // profile hook (bench.py roofline.attention): QK^T + PV = 4 T^2 C flop per image (12.18 GFLOP per forward)
        const double T = (double)x.H * x.W;
        PD_TRY(prof_begin(c, 4.0 * c.N * T * T * x.C, 1));
        PD_TRY(attention(qkv.p, a.p, c.N, x.H * x.W, x.C, c.u->head, c.s, vt, c.t.attn_nbuf, c.t.attn_qtn, c.t.attn_vt));
        PD_TRY(prof_end(c));
    }
    return run_conv(c, ab.name + ".proj_out", plan_conv(c, a, ab.proj, true), ab.proj, ConvIn{&a, x.p}, out);
}

int run_blocks(Ctx& c, std::vector<Block>& blocks, Act* h, const float* x_nchw) {
    for (Block& b : blocks) {
        Act o;
        if (b.kind == 0) {
            o.C = c.u->mult[0] * c.u->mc; o.H = o.W = c.u->image_size;
            const int cpad = ((o.C + 127) / 128) * 128;
            ConvNeeds nd;
            nd.want_gn = true;
            const ConvPlan p = conv_plan(c.t, c.N, o.H, o.W, 32, o.C, cpad, 1, nd, 0);      // the 1x1 conv over the im2col rows conv_in_3x3 launches (no workspace)
            o.p = arena_take(c.u, (size_t)c.N * o.H * o.W * o.C);
            half_t* col = arena_take(c.u, (size_t)c.N * o.H * o.W * 32);
            float* part = reinterpret_cast<float*>(arena_take(c.u, (size_t)c.N * ((o.H * o.W + 127) / 128) * (o.C / 8) * 2 * 2));
            if (c.table) { Act in{nullptr, 32, o.H, o.W}; table_row(c, "input_blocks.0.0", p, ConvIn{&in}, &o); }
            if (!c.dry) adopt_parts(&o, part, p.gn_chunks);
            if (c.go()) {
                PD_REQUIRE(c.u->have_win && c.u->have_bin, "unet: input conv not loaded");
                PD_TRY(conv_in_3x3(p, x_nchw, c.u->w_in, c.u->b_in, o.p, c.N, o.H, o.W, o.C, cpad, col, c.u->zero_page, c.s, part));
            }
        } else if (b.kind == 1) {
            PD_TRY(run_res(c, *h, c.u->res[b.idx], &o));
        } else {
            PD_TRY(run_att(c, *h, c.u->att[b.idx], &o));
        }
        *h = o;
    }
    return PDHIP_OK;
}

// the whole forward; dry = sizing pass (no launches); table != NULL = planning only (real routing, no launches, one line per conv)
// shared_emb: one precomputed row of ResBlock embeddings [emb_rows] used by every image (t is then ignored), or nullptr
// tun: the hooks in force, taken from the calling thread's instance by the entry point
int forward_impl(const Tuning& tun, pdhip_unet* u, const float* x, const float* t, int N, float* out, hipStream_t s, bool dry,
                 const float* shared_emb = nullptr, int head_ch = 0, Table* table = nullptr) {   // head_ch 3: only eps (out [N,3,H,W]); 0 = all out_ch
    Ctx c{u, N, s, dry, shared_emb ? shared_emb : u->emb_all, shared_emb ? 0 : u->emb_rows, table, tun};
    u->arena_off = 0;
    u->arena_overflow = false;
    if (c.go() && u->prof.on) u->prof.armed = (u->prof.forwards++ % u->prof.period) == 0;      // events around every period-th forward's launches
    if (c.go() && shared_emb == nullptr) {
        PD_REQUIRE(u->have_te[0] && u->have_te[1] && u->have_te[2] && u->have_te[3], "unet: time_embed not loaded");
        PD_TRY(timestep_mlp(t, N, u->mc, u->te_w0, u->te_b0, u->te_w2, u->te_b2, u->emb_silu, u->emb_tmp, s));
        PD_TRY(gemv_rows(u->emb_w, u->emb_b, u->emb_silu, u->emb_all, (int)u->emb_rows, u->ted, N, s));
    }
    std::vector<Act> hs;
    Act h{nullptr, 0, 0, 0};
    for (auto& blk : u->input) {
        PD_TRY(run_blocks(c, blk, &h, x));
        hs.push_back(h);
    }
    PD_TRY(run_blocks(c, u->middle, &h, x));
    for (auto& blk : u->output) {
        Act sk = hs.back(); hs.pop_back();
        // torch.cat([h, skip], dim=1): when both tensors carry fused GroupNorm partials (and 64-channel granularity for the
        // 1x1 skip conv's K loop) the concat stays virtual -- its two consumers (GroupNorm apply, skip conv) read both tensors
        Act cat{nullptr, h.C + sk.C, h.H, h.W};
        const bool part_ok = h.gn_part && sk.gn_part && !h.gn_partB && !sk.gn_partB && !h.p2 && !sk.p2;
        if (part_ok) {
            cat.gn_part = h.gn_part; cat.gn_partB = sk.gn_part; cat.Ca = h.C; cat.gn_chunks = h.gn_chunks; cat.gn_chunksB = sk.gn_chunks;
            cat.row = h.row; cat.rowB = sk.row;
        }
        const Block& first = blk.front();
        const bool virt = part_ok && h.C % 64 == 0 && sk.C % 64 == 0 && ((cat.C / 32) % 8) == 0 && first.kind == 1 &&
                          u->res[first.idx].mode == 0 && u->res[first.idx].has_skip;
        if (virt) {
            cat.p = h.p; cat.p2 = sk.p;
        } else {
            cat.p = arena_take(u, (size_t)N * h.H * h.W * (h.C + sk.C));
            if (c.go()) PD_TRY(concat_channels(h.p, h.C, sk.p, sk.C, (long long)N * h.H * h.W, cat.p, s));
        }
        h = cat;
        PD_TRY(run_blocks(c, blk, &h, x));
    }
    if (c.go()) {
        PD_REQUIRE(!u->arena_overflow, "unet: activation arena too small for this routing (sized at create())");
        PD_REQUIRE(u->out_norm.have_g && u->out_norm.have_b && u->have_ow && u->have_ob, "unet: output head not loaded");
        PD_TRY(run_gn_stats(c, h));
        const bool eps_only = head_ch == 3 && u->out_ch == 6;
        PD_TRY(head_gn_silu_conv3x3(h.p, u->stats, u->out_norm.g, u->out_norm.b, eps_only ? u->head_wz3 : u->head_wz, u->out_b, out, N,
                                    h.H, h.W, h.C, eps_only ? 3 : u->out_ch, s));
    }
    return PDHIP_OK;
}

// ---- graph (unet.py:481-617): host only.  Every conv gets its shape here, and routing's "do the packed copies exist" questions their answers
// (has_wf, has_wph, has_c2s, has_c2s_wf); pdhip_unet_create allocates what they say, pdhip_unet_route_table plans without a device.
const size_t kSplitkFloats = (size_t)16 * 384 * 128 * 128;               // 16 splits x (< 384 tiles of 128x128) f32
void shape_conv(ConvW& c, int cin, int cout, int taps) { c.cin = cin; c.cout = cout; c.taps = taps; c.cout_pad = ((cout + 127) / 128) * 128; }
int build_graph(pdhip_unet* u, int image_size, int model_channels, int num_res_blocks, const int* channel_mult, int n_mult,
                const int* attention_ds, int n_att, int num_head_channels, int out_channels, int max_batch) {
    PD_REQUIRE(channel_mult && n_mult > 0 && (n_att == 0 || attention_ds), "pdhip_unet_create: null argument");
    PD_REQUIRE(model_channels % 32 == 0 && image_size % (1 << (n_mult - 1)) == 0 && max_batch >= 1 && max_batch <= 64,
               "pdhip_unet_create: model_channels %% 32, image_size %% 2^(levels-1), 1 <= max_batch <= 64 required");
    PD_REQUIRE(num_head_channels == 32 || num_head_channels == 64, "pdhip_unet_create: num_head_channels must be 32 or 64");
    PD_REQUIRE(out_channels == 3 || out_channels == 6, "pdhip_unet_create: out_channels must be 3 or 6");
    u->image_size = image_size; u->mc = model_channels; u->nres = num_res_blocks; u->head = num_head_channels;
    u->out_ch = out_channels; u->max_batch = max_batch; u->ted = model_channels * 4;
    u->splitk_floats = kSplitkFloats;
    u->mult.assign(channel_mult, channel_mult + n_mult);
    u->att_ds.assign(attention_ds, attention_ds + n_att);
    auto is_att = [&](int ds) { for (int a : u->att_ds) if (a == ds) return true; return false; };
    long long emb_rows = 0;
    auto add_res = [&](const std::string& name, int cin, int cout, int mode, int hw) -> int {
        ResB rb; rb.name = name; rb.cin = cin; rb.cout = cout; rb.mode = mode; rb.has_skip = cin != cout; rb.hw = hw;
        rb.emb_off = emb_rows; emb_rows += 2 * cout;
        shape_conv(rb.c1, cin, cout, 9); shape_conv(rb.c2, cout, cout, 9);
        if (rb.has_skip) shape_conv(rb.skip, cin, cout, 1);
        rb.has_c2s = rb.has_skip && mode == 0 && cin % 64 == 0 && cout % 64 == 0;       // fused [conv2 | skip] weights
        // phase weights of an up block's in_layers conv, 16 Cin Cout_pad f16 (50 MB over the four up blocks whose half-resolution image holds whole 256-pixel tiles)
        rb.c1.has_wph = mode == 2 && ((hw / 2) * (hw / 2)) % 256 == 0 && conv_up2_phase_eligible(1, hw / 2, hw / 2, cin, cout, rb.c1.cout_pad);
        // fragment-major copies for the row-resident kernel (small-batch route of the <= 64^2 levels; +~1 GB at the 256^2 config: 288 GB HBM)
        rb.c1.has_wf = rb.c2.has_wf = hw <= 64 && cin % 128 == 0 && cout % 128 == 0;
        rb.has_c2s_wf = rb.c2.has_wf && rb.has_c2s;
        u->res.push_back(rb);
        return (int)u->res.size() - 1;
    };
    auto add_att = [&](const std::string& name, int c) -> int {
        AttB ab; ab.name = name; ab.c = c;
        shape_conv(ab.qkv, c, 3 * c, 1); shape_conv(ab.proj, c, c, 1);
        u->att.push_back(ab);
        return (int)u->att.size() - 1;
    };
    int ch = u->mult[0] * u->mc;
    std::vector<int> chans{ch};
    u->input.push_back({Block{0, 0}});
    int ds = 1, n = 1;
    for (int level = 0; level < n_mult; ++level) {
        for (int r = 0; r < num_res_blocks; ++r) {
            std::vector<Block> layers;
            const int o = u->mult[level] * u->mc;
            layers.push_back(Block{1, add_res("input_blocks." + std::to_string(n) + ".0", ch, o, 0, image_size / ds)});
            ch = o;
            if (is_att(ds)) layers.push_back(Block{2, add_att("input_blocks." + std::to_string(n) + ".1", ch)});
            u->input.push_back(layers);
            chans.push_back(ch);
            ++n;
        }
        if (level != n_mult - 1) {
            u->input.push_back({Block{1, add_res("input_blocks." + std::to_string(n) + ".0", ch, ch, 1, image_size / (ds * 2))}});
            chans.push_back(ch);
            ds *= 2;
            ++n;
        }
    }
    u->middle.push_back(Block{1, add_res("middle_block.0", ch, ch, 0, image_size / ds)});
    u->middle.push_back(Block{2, add_att("middle_block.1", ch)});
    u->middle.push_back(Block{1, add_res("middle_block.2", ch, ch, 0, image_size / ds)});
    n = 0;
    for (int level = n_mult - 1; level >= 0; --level) {
        for (int i = 0; i < num_res_blocks + 1; ++i) {
            const int ich = chans.back(); chans.pop_back();
            const int o = u->mc * u->mult[level];
            std::vector<Block> layers;
            const std::string base = "output_blocks." + std::to_string(n) + ".";
            layers.push_back(Block{1, add_res(base + "0", ch + ich, o, 0, image_size / ds)});
            ch = o;
            int k = 1;
            if (is_att(ds)) { layers.push_back(Block{2, add_att(base + std::to_string(k), ch)}); ++k; }
            if (level && i == num_res_blocks) {
                layers.push_back(Block{1, add_res(base + std::to_string(k), ch, ch, 2, image_size / (ds / 2))});
                ds /= 2;
            }
            u->output.push_back(layers);
            ++n;
        }
    }
    u->final_ch = ch;
    u->emb_rows = emb_rows;
    return PDHIP_OK;
}

}  // namespace

// =================================================================================================
extern "C" int pdhip_unet_create(int image_size, int model_channels, int num_res_blocks, const int* channel_mult, int n_mult,
                                 const int* attention_ds, int n_att, int num_head_channels, int out_channels, int max_batch,
                                 pdhip_unet** out) {
    PD_REQUIRE(out, "pdhip_unet_create: null argument");
    pdhip_unet* u = new pdhip_unet();
    *out = nullptr;
    auto fail = [&](int rc) { for (void* p : u->owned) (void)hipFree(p); delete u; return rc; };
    int rc = build_graph(u, image_size, model_channels, num_res_blocks, channel_mult, n_mult, attention_ds, n_att, num_head_channels, out_channels, max_batch);
    if (rc) return fail(rc);
    const long long emb_rows = u->emb_rows;
    // ---- parameters
    auto chk = [&](int r) { if (rc == PDHIP_OK) rc = r; };
    for (ResB& rb : u->res) {
        chk(alloc_norm(u, rb.n1, rb.cin)); chk(alloc_norm(u, rb.n2, rb.cout));
        chk(alloc_conv(u, rb.c1)); chk(alloc_conv(u, rb.c2));
        if (rb.has_skip) chk(alloc_conv(u, rb.skip));
        if (rb.has_c2s) {       // (filled by pdhip_unet_load_tensor once its four sources are loaded)
            chk(dalloc(u, &rb.c2s_w, (size_t)rb.c2.cout_pad * (9 * (size_t)rb.cout + rb.cin)));
            chk(dalloc(u, &rb.c2s_b, (size_t)rb.cout));
        }
        if (rb.c1.has_wph) chk(dalloc(u, &rb.c1.wph, (size_t)16 * rb.c1.cout_pad * rb.cin));
        if (rb.c1.has_wf) chk(dalloc(u, &rb.c1.wf, conv_rr_weight_halfs(rb.cin, 9, 0, rb.cout)));
        if (rb.c2.has_wf) chk(dalloc(u, &rb.c2.wf, conv_rr_weight_halfs(rb.cout, 9, 0, rb.cout)));
        if (rb.has_c2s_wf) chk(dalloc(u, &rb.c2s_wf, conv_rr_weight_halfs(rb.cout, 9, rb.cin, rb.cout)));
        if (rc) return fail(rc);
    }
    for (AttB& ab : u->att) {
        chk(alloc_norm(u, ab.n, ab.c)); chk(alloc_conv(u, ab.qkv)); chk(alloc_conv(u, ab.proj));
        if (rc) return fail(rc);
    }
    const int c0 = u->mult[0] * u->mc;
    chk(dalloc(u, &u->w_in, (size_t)(((c0 + 127) / 128) * 128) * 32)); chk(dalloc(u, &u->b_in, (size_t)c0));
    if (rc == PDHIP_OK && hipMemset(u->w_in, 0, (size_t)(((c0 + 127) / 128) * 128) * 32 * sizeof(half_t)) != hipSuccess) rc = PDHIP_E_HIP;
    chk(dalloc(u, &u->te_w0, (size_t)u->ted * u->mc)); chk(dalloc(u, &u->te_b0, (size_t)u->ted));
    chk(dalloc(u, &u->te_w2, (size_t)u->ted * u->ted)); chk(dalloc(u, &u->te_b2, (size_t)u->ted));
    chk(dalloc(u, &u->emb_w, (size_t)emb_rows * u->ted)); chk(dalloc(u, &u->emb_b, (size_t)emb_rows));
    chk(alloc_norm(u, u->out_norm, u->final_ch));
    chk(dalloc(u, &u->out_w, (size_t)out_channels * 9 * u->final_ch)); chk(dalloc(u, &u->out_b, (size_t)out_channels));
    chk(dalloc(u, &u->zero_page, (size_t)128));
    if (rc) return fail(rc);
    if (hipMemset(u->zero_page, 0, 256) != hipSuccess) { set_error("hipMemset failed"); return fail(PDHIP_E_HIP); }
    // ---- workspace (sized by a dry run of the forward at max_batch)
    const size_t S2 = (size_t)image_size * image_size;
    chk(forward_impl(tuning(), u, nullptr, nullptr, max_batch, nullptr, nullptr, true));
    u->arena_bytes = u->arena_off + 4096;
    {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, u->arena_bytes);
        if (e != hipSuccess) { set_error("pdhip_unet_create: activation arena of %zu bytes: %s", u->arena_bytes, hipGetErrorString(e)); return fail(PDHIP_E_NOMEM); }
        u->owned.push_back(q);
        u->arena = reinterpret_cast<char*>(q);
    }
    u->gn_ws_floats = (size_t)max_batch * ((S2 + 255) / 256) * 64;
    chk(dalloc(u, &u->stats, (size_t)max_batch * 64)); chk(dalloc(u, &u->gn_ws, u->gn_ws_floats));
    { int cmax = 0; for (const ResB& rb : u->res) cmax = std::max(cmax, std::max(rb.cin, rb.cout)); chk(dalloc(u, &u->ap_table, (size_t)max_batch * cmax * 2)); }
    chk(dalloc(u, &u->emb_silu, (size_t)max_batch * u->ted)); chk(dalloc(u, &u->emb_tmp, (size_t)max_batch * (u->mc + u->ted)));
    chk(dalloc(u, &u->emb_all, (size_t)max_batch * emb_rows));
    chk(dalloc(u, &u->steps_t, 128)); chk(dalloc(u, &u->steps_silu, (size_t)100 * u->ted));
    chk(dalloc(u, &u->steps_tmp, (size_t)100 * (u->mc + u->ted))); chk(dalloc(u, &u->steps_emb, (size_t)100 * emb_rows));
    { float* wz = nullptr; chk(dalloc(u, &wz, (size_t)64 * u->final_ch)); u->head_wz = reinterpret_cast<half_t*>(wz); }
    { float* wz = nullptr; chk(dalloc(u, &wz, (size_t)64 * u->final_ch)); u->head_wz3 = reinterpret_cast<half_t*>(wz); }
    chk(dalloc(u, &u->t_dev, (size_t)max_batch));
    chk(dalloc(u, &u->splitk_ws, u->splitk_floats));
    if (rc == PDHIP_OK && hipMemset(u->splitk_ws, 0, PD_SK_TICKET_FLOATS * sizeof(float)) != hipSuccess) rc = PDHIP_E_HIP;   // k_conv_sk's tickets
    chk(dalloc(u, &u->sx, (size_t)max_batch * 3 * S2)); chk(dalloc(u, &u->sy, (size_t)max_batch * 3 * S2));
    chk(dalloc(u, &u->set_, (size_t)max_batch * out_channels * S2)); chk(dalloc(u, &u->smask, (size_t)max_batch * S2));
    if (rc) return fail(rc);
    *out = u;
    return PDHIP_OK;
}

extern "C" void pdhip_unet_destroy(pdhip_unet* u) {
    if (!u) return;
    for (hipEvent_t e : u->prof.ev) (void)hipEventDestroy(e);
    for (void* p : u->owned) (void)hipFree(p);
    delete u;
}

extern "C" long long pdhip_unet_arena_bytes(const pdhip_unet* u) { return u ? (long long)u->arena_bytes : -1; }

// host-only: the route of every conv of a batch-N forward of the network pdhip_unet_create would build from the same arguments, under the hooks
// in force -- the forward walked in planning mode (real routing, nothing allocated, nothing launched).  One line per conv, in launch order:
//   <layer> <H>x<W> <Cin>-><Cout> <kernel> <splits / slabs / variant> gn=<chunks per image> <folds taken, or ->
// Returns the length of the whole table (a negative error code on bad arguments); buf (may be NULL) gets as much of it as fits, NUL-terminated.
extern "C" int pdhip_unet_route_table(int image_size, int model_channels, int num_res_blocks, const int* channel_mult, int n_mult,
                                      const int* attention_ds, int n_att, int num_head_channels, int out_channels, int max_batch, int N,
                                      char* buf, int buf_len) {
    pdhip_unet u;
    int rc = build_graph(&u, image_size, model_channels, num_res_blocks, channel_mult, n_mult, attention_ds, n_att, num_head_channels, out_channels, max_batch);
    if (rc == PDHIP_OK && (N < 1 || N > max_batch)) { set_error("pdhip_unet_route_table: batch %d outside [1, %d]", N, max_batch); rc = PDHIP_E_ARG; }
    if (rc != PDHIP_OK) return rc;
    u.arena = reinterpret_cast<char*>((size_t)1 << 20);      // addresses to tell "has a tensor" from "has none" by; never dereferenced
    u.arena_bytes = ~(size_t)0 >> 1;
    Table table;
    rc = forward_impl(tuning(), &u, nullptr, nullptr, N, nullptr, nullptr, false, nullptr, 0, &table);
    if (rc != PDHIP_OK) return rc;
    std::string all;
    for (const std::string& l : table.line) { all += l; all += '\n'; }
    if (buf && buf_len > 0) { strncpy(buf, all.c_str(), buf_len - 1); buf[buf_len - 1] = 0; }
    return (int)all.size();
}

// names still missing after loading (count); if buf != NULL the first names are written, '\n'-separated
extern "C" int pdhip_unet_missing_tensors(const pdhip_unet* u, char* buf, int buf_len) {
    if (!u) return -1;
    std::vector<std::string> miss;
    auto conv = [&](const std::string& n, const ConvW& c) { if (!c.have_w) miss.push_back(n + ".weight"); if (!c.have_b) miss.push_back(n + ".bias"); };
    auto norm = [&](const std::string& n, const NormW& c) { if (!c.have_g) miss.push_back(n + ".weight"); if (!c.have_b) miss.push_back(n + ".bias"); };
    if (!u->have_win) miss.push_back("input_blocks.0.0.weight");
    if (!u->have_bin) miss.push_back("input_blocks.0.0.bias");
    const char* te[4] = {"time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight", "time_embed.2.bias"};
    for (int i = 0; i < 4; ++i) if (!u->have_te[i]) miss.push_back(te[i]);
    for (const ResB& rb : u->res) {
        norm(rb.name + ".in_layers.0", rb.n1); conv(rb.name + ".in_layers.2", rb.c1);
        if (!rb.have_ew) miss.push_back(rb.name + ".emb_layers.1.weight");
        if (!rb.have_eb) miss.push_back(rb.name + ".emb_layers.1.bias");
        norm(rb.name + ".out_layers.0", rb.n2); conv(rb.name + ".out_layers.3", rb.c2);
        if (rb.has_skip) conv(rb.name + ".skip_connection", rb.skip);
    }
    for (const AttB& ab : u->att) { norm(ab.name + ".norm", ab.n); conv(ab.name + ".qkv", ab.qkv); conv(ab.name + ".proj_out", ab.proj); }
    norm("out.0", u->out_norm);
    if (!u->have_ow) miss.push_back("out.2.weight");
    if (!u->have_ob) miss.push_back("out.2.bias");
    if (buf && buf_len > 0) {
        std::string s;
        for (const std::string& m : miss) { if ((int)(s.size() + m.size() + 2) >= buf_len) break; s += m; s += '\n'; }
        strncpy(buf, s.c_str(), buf_len - 1); buf[buf_len - 1] = 0;
    }
    return (int)miss.size();
}

extern "C" int pdhip_unet_num_tensors(const pdhip_unet* u) {
    if (!u) return -1;
    int n = 2 + 4 + 4;                                   // conv_in, time_embed, out.0/out.2
    for (const ResB& rb : u->res) n += 10 + (rb.has_skip ? 2 : 0);
    n += 6 * (int)u->att.size();
    return n;
}

extern "C" int pdhip_unet_load_tensor(pdhip_unet* u, const char* name_c, const void* data, int is_f16, const int64_t* shape,
                                      int ndim, void* stream) {
    PD_REQUIRE(u && name_c && data && shape && ndim >= 1 && ndim <= 4, "pdhip_unet_load_tensor: bad arguments");
    u->steps_cached = 0;                         // any weight change invalidates the sampler's per-step embedding table
    hipStream_t s = as_stream(stream);
    const std::string name(name_c);
    long long numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= shape[i];
    auto want = [&](long long n, const char* what) -> int {
        PD_REQUIRE(numel == n, "pdhip_unet_load_tensor: %s: %s expects %lld elements, got %lld", name_c, what, n, numel);
        return PDHIP_OK;
    };
    auto load_vec = [&](float* dst, long long n, bool* flag, int round16) -> int {
        PD_TRY(want(n, "vector"));
        k_copy_f32<<<grid_for(n), 256, 0, s>>>(data, is_f16, n, dst, round16);
        PD_LAUNCH_CHECK();
        *flag = true;
        return PDHIP_OK;
    };
    auto load_conv_w = [&](ConvW& c) -> int {
        PD_TRY(want((long long)c.cout * c.cin * c.taps, "conv weight"));
        PD_REQUIRE(shape[0] == c.cout && shape[1] == c.cin, "pdhip_unet_load_tensor: %s: shape mismatch", name_c);
        k_pack_conv<<<grid_for(numel), 256, 0, s>>>(data, is_f16, c.cout, c.cin, c.taps, c.w);
        PD_LAUNCH_CHECK();
        if (c.has_wf) PD_TRY(conv_rr_pack(c.w, c.cin, c.taps, 0, c.cout, c.wf, s));      // (same stream: ordered behind the repack above)
        if (c.has_wph) PD_TRY(conv_up2_phase_pack(c.w, c.cin, c.cout_pad, c.wph, s));   // (from the f16-rounded taps: an f32 and an f16 checkpoint give the same bytes)
        c.have_w = true;
        return PDHIP_OK;
    };
    auto ends = [&](const std::string& suf) { return name.size() >= suf.size() && name.compare(name.size() - suf.size(), suf.size(), suf) == 0; };
    auto starts = [&](const std::string& pre) { return name.compare(0, pre.size(), pre) == 0; };
    if (name == "input_blocks.0.0.weight") {
        const int c0 = u->mult[0] * u->mc;
        PD_TRY(want((long long)c0 * 27, "input conv weight"));
        k_pack_conv_in<<<grid_for(numel), 256, 0, s>>>(data, is_f16, c0, u->w_in);
        PD_LAUNCH_CHECK();
        u->have_win = true;
        return PDHIP_OK;
    }
    if (name == "input_blocks.0.0.bias") return load_vec(u->b_in, u->mult[0] * u->mc, &u->have_bin, 1);
    if (name == "time_embed.0.weight") return load_vec(u->te_w0, (long long)u->ted * u->mc, &u->have_te[0], 0);
    if (name == "time_embed.0.bias") return load_vec(u->te_b0, u->ted, &u->have_te[1], 0);
    if (name == "time_embed.2.weight") return load_vec(u->te_w2, (long long)u->ted * u->ted, &u->have_te[2], 0);
    if (name == "time_embed.2.bias") return load_vec(u->te_b2, u->ted, &u->have_te[3], 0);
    if (name == "out.0.weight") return load_vec(u->out_norm.g, u->final_ch, &u->out_norm.have_g, 0);
    if (name == "out.0.bias") return load_vec(u->out_norm.b, u->final_ch, &u->out_norm.have_b, 0);
    if (name == "out.2.bias") return load_vec(u->out_b, u->out_ch, &u->have_ob, 0);
    if (name == "out.2.weight") {
        PD_TRY(want((long long)u->out_ch * u->final_ch * 9, "out conv weight"));
        k_pack_conv_f32<<<grid_for(numel), 256, 0, s>>>(data, is_f16, u->out_ch, u->final_ch, 9, u->out_w);
        PD_LAUNCH_CHECK();
        PD_TRY(head_pack(u->out_w, u->out_ch, u->final_ch, u->head_wz, s));
        PD_TRY(head_pack(u->out_w, 3, u->final_ch, u->head_wz3, s));            // rows 0..2 of [out_ch][9 C]
        u->have_ow = true;
        return PDHIP_OK;
    }
    for (ResB& rb : u->res) {
        if (!starts(rb.name + ".")) continue;
        const std::string rest = name.substr(rb.name.size() + 1);
        if (rest == "in_layers.0.weight") return load_vec(rb.n1.g, rb.cin, &rb.n1.have_g, 0);
        if (rest == "in_layers.0.bias") return load_vec(rb.n1.b, rb.cin, &rb.n1.have_b, 0);
        if (rest == "in_layers.2.weight") return load_conv_w(rb.c1);
        if (rest == "in_layers.2.bias") return load_vec(rb.c1.b, rb.cout, &rb.c1.have_b, 1);
        if (rest == "emb_layers.1.weight") return load_vec(u->emb_w + rb.emb_off * u->ted, (long long)2 * rb.cout * u->ted, &rb.have_ew, 0);
        if (rest == "emb_layers.1.bias") return load_vec(u->emb_b + rb.emb_off, 2 * rb.cout, &rb.have_eb, 0);
        if (rest == "out_layers.0.weight") return load_vec(rb.n2.g, rb.cout, &rb.n2.have_g, 0);
        if (rest == "out_layers.0.bias") return load_vec(rb.n2.b, rb.cout, &rb.n2.have_b, 0);
        // The fused [conv2 | skip] copy of conv_sk_skip is (re)built HERE, on the loading stream, as soon as its four source tensors are
        // present (built lazily inside the first forward it could be merely RECORDED by a HIP-graph capture, and an eager
        // forward issued before the replay would have read uninitialised weights).
        auto refuse = [&](int rc) -> int {
            if (rc != PDHIP_OK || !rb.has_c2s) return rc;
            rb.c2s_ready = false;
            if (rb.c2.have_w && rb.c2.have_b && rb.skip.have_w && rb.skip.have_b && rb.skip.taps == 1) {
                PD_TRY(fuse_skip_weights(rb.c2.w, 9 * rb.c2.cin, rb.skip.w, rb.skip.cin, rb.c2.cout_pad, rb.c2.b, rb.skip.b, rb.cout, rb.c2s_w, rb.c2s_b, s));
                if (rb.has_c2s_wf) PD_TRY(conv_rr_pack(rb.c2s_w, rb.c2.cin, 9, rb.skip.cin, rb.cout, rb.c2s_wf, s));
                rb.c2s_ready = true;
            }
            return PDHIP_OK;
        };
        if (rest == "out_layers.3.weight") return refuse(load_conv_w(rb.c2));
        if (rest == "out_layers.3.bias") return refuse(load_vec(rb.c2.b, rb.cout, &rb.c2.have_b, 1));
        if (rb.has_skip && rest == "skip_connection.weight") return refuse(load_conv_w(rb.skip));
        if (rb.has_skip && rest == "skip_connection.bias") return refuse(load_vec(rb.skip.b, rb.cout, &rb.skip.have_b, 1));
    }
    for (AttB& ab : u->att) {
        if (!starts(ab.name + ".")) continue;
        const std::string rest = name.substr(ab.name.size() + 1);
        if (rest == "norm.weight") return load_vec(ab.n.g, ab.c, &ab.n.have_g, 0);
        if (rest == "norm.bias") return load_vec(ab.n.b, ab.c, &ab.n.have_b, 0);
        if (rest == "qkv.weight") return load_conv_w(ab.qkv);
        if (rest == "qkv.bias") return load_vec(ab.qkv.b, 3 * ab.c, &ab.qkv.have_b, 1);
        if (rest == "proj_out.weight") return load_conv_w(ab.proj);
        if (rest == "proj_out.bias") return load_vec(ab.proj.b, ab.c, &ab.proj.have_b, 1);
    }
    (void)ends;
    set_error("pdhip_unet_load_tensor: unknown tensor name '%s'", name_c);
    return PDHIP_E_UNKNOWN_NAME;
}

extern "C" int pdhip_unet_forward(pdhip_unet* u, const float* x, const float* t, int N, float* out, void* stream) {
    PD_REQUIRE(u && x && t && out, "pdhip_unet_forward: null argument");
    PD_REQUIRE(N >= 1 && N <= u->max_batch, "pdhip_unet_forward: batch %d outside [1, %d]", N, u->max_batch);
    return forward_impl(tuning(), u, x, t, N, out, as_stream(stream), false);
}

// ---- profiling of the dominant kernel (3x3 implicit-GEMM launches) with HIP events on the launch stream
extern "C" int pdhip_unet_profile(pdhip_unet* u, int enable) {
    PD_REQUIRE(u, "pdhip_unet_profile: null handle");
    u->prof.on = enable != 0;                      // enable = k > 1: only every k-th forward carries events (an event record is a
    u->prof.period = enable > 1 ? enable : 1;      // barrier packet: ~5 us of pipeline bubble each, 108 per forward)
    u->prof.forwards = 0;
    u->prof.armed = false;
    u->prof.used = 0;
    u->prof.flops[0] = u->prof.flops[1] = 0;
    return PDHIP_OK;
}
static int prof_read(pdhip_unet* u, int cls, double* total_ms, double* total_flops, long long* launches) {
    double ms = 0;
    long long n = 0;
    for (size_t i = 0; i + 1 < u->prof.used; i += 2) {
        if (u->prof.cls[i] != cls) continue;
        PD_HIP(hipEventSynchronize(u->prof.ev[i + 1]));
        float e = 0;
        PD_HIP(hipEventElapsedTime(&e, u->prof.ev[i], u->prof.ev[i + 1]));
        ms += e; ++n;
    }
    *total_ms = ms; *total_flops = u->prof.flops[cls]; *launches = n;
    return PDHIP_OK;
}
extern "C" int pdhip_unet_profile_read(pdhip_unet* u, double* total_ms, double* total_flops, long long* launches) {
    PD_REQUIRE(u && total_ms && total_flops && launches, "pdhip_unet_profile_read: null argument");
    return prof_read(u, 0, total_ms, total_flops, launches);
}
/* the same for the attention launches (k_attention_t64 + its V transpose / k_attention): 4 T^2 C flop per image */
extern "C" int pdhip_unet_profile_read_attention(pdhip_unet* u, double* total_ms, double* total_flops, long long* launches) {
    PD_REQUIRE(u && total_ms && total_flops && launches, "pdhip_unet_profile_read_attention: null argument");
    return prof_read(u, 1, total_ms, total_flops, launches);
}

// ---- D1: DDNM schedule (diffusion.py:46-113, 770-812) computed on the host exactly as the reference forms it
namespace {
struct Sched { std::vector<int> t; std::vector<DdnmCoef> co; std::vector<float> ab; };
Sched make_schedule() {
    // betas = np.linspace(1e-4, 0.02, 1000) (f64: start + i*step, last = stop) -> f32;
    // alpha_bar(t) = cumprod(1 - [0, beta])[t+1] on f32 inputs; torch's CPU cumprod accumulates in f64 and rounds
    // each prefix to f32 (the golden vectors pin exactly this; a CUDA scan differs in the last ulp).
    Sched s;
    s.ab.resize(1001);
    double acc = 1.0;
    s.ab[0] = 1.0f;                                                // index t+1 with t = -1
    const double b0 = 1e-4, b1 = 0.02, step = (b1 - b0) / 999.0;
    for (int i = 0; i < 1000; ++i) {
        const double beta = (i == 999) ? b1 : b0 + (double)i * step;
        acc = acc * (double)(1.0f - (float)beta);
        s.ab[i + 1] = (float)acc;
    }
    const double eta = 0.85;
    for (int k = 99; k >= 0; --k) {
        const int t = k * 10, tn = (k - 1) * 10 < 0 ? -1 : (k - 1) * 10;
        const float at = s.ab[t + 1], an = s.ab[tn + 1];
        DdnmCoef c;
        c.sqrt_1m_at = sqrtf(1.0f - at); c.sqrt_at = sqrtf(at); c.sqrt_at_next = sqrtf(an);
        c.sigma_t = sqrtf(1.0f - an * an);
        c.c1 = sqrtf(1.0f - an) * (float)eta;
        c.c2 = sqrtf(1.0f - an) * (float)std::sqrt(1.0 - eta * eta);
        s.t.push_back(t); s.co.push_back(c);
    }
    return s;
}
__global__ void k_fill(float* p, float v, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }
}  // namespace

extern "C" int pdhip_ddnm_schedule(float* at, float* at_next, int* t, int* t_next, float* coefs /*[100][6]*/) {
    Sched s = make_schedule();
    for (int k = 0; k < 100; ++k) {
        const int tt = s.t[k], tn = tt - 10 < 0 ? -1 : tt - 10;
        if (at) at[k] = s.ab[tt + 1];
        if (at_next) at_next[k] = s.ab[tn + 1];
        if (t) t[k] = tt;
        if (t_next) t_next[k] = tn;
        if (coefs) memcpy(coefs + 6 * k, &s.co[k], sizeof(DdnmCoef));
    }
    return PDHIP_OK;
}

extern "C" int pdhip_ddnm_step(float* x, const float* et, int et_channels, const float* y, const float* mask, const float* eps,
                               uint64_t seed, int step, int N, int HW, void* stream) {
    PD_REQUIRE(x && et && y && mask && step >= 0 && step < 100 && (et_channels == 3 || et_channels == 6), "pdhip_ddnm_step: bad arguments");
    static const Sched sched = make_schedule();
    return ddnm_update(x, et, et_channels, y, mask, eps, seed, (unsigned long long)step + 1, sched.co[step], N, HW, as_stream(stream));
}

extern "C" int pdhip_ddnm_prepare(const float* masked_imgs, const float* masks, float* y, int N, int HW, void* stream) {
    PD_REQUIRE(masked_imgs && masks && y, "pdhip_ddnm_prepare: null argument");
    return ddnm_prepare(masked_imgs, masks, y, N, HW, as_stream(stream));
}

// The whole of simplified_ddnm_inpainting for N images at once: no host round trip inside the loop.
// x_T / eps_tape (eps_tape[k] = noise of step k, [n_steps,N,3,S,S]) may be NULL -> Philox noise from `seed`.
// first_image_key: image n of the batch draws the Philox noise stream of key first_image_key + n (x_T: stream 0, step k: stream
// k + 1, counter = key * 3HW/4 + element / 4): the noise of a view does not depend on its position in the batch, on the batch
// it shares a sampler call with, or on how the views of a shape are sharded over ranks.
extern "C" int pdhip_ddnm_sample_keyed(pdhip_unet* u, const float* masked_imgs, const float* masks, int N, const float* x_T,
                                       const float* eps_tape, uint64_t seed, uint64_t first_image_key, int n_steps, float* out,
                                       void* stream) {
    PD_REQUIRE(u && masked_imgs && masks && out, "pdhip_ddnm_sample: null argument");
    PD_REQUIRE(N >= 1 && N <= u->max_batch && n_steps >= 1 && n_steps <= 100, "pdhip_ddnm_sample: bad N / n_steps");
    static const Sched sched = make_schedule();
    hipStream_t s = as_stream(stream);
    const int HW = u->image_size * u->image_size;
    const long long n3 = (long long)N * 3 * HW;
    PD_TRY(ddnm_prepare(masked_imgs, masks, u->sy, N, HW, s));
    const unsigned long long quad0 = (unsigned long long)first_image_key * (unsigned long long)(3LL * HW / 4);
    if (x_T) PD_HIP(hipMemcpyAsync(u->sx, x_T, n3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    else PD_TRY(philox_normal(u->sx, n3, seed, 0, s, quad0));
    if (u->steps_cached != n_steps) {            // embeddings of every schedule step, one pass over the emb_layers weights
        PD_REQUIRE(u->have_te[0] && u->have_te[1] && u->have_te[2] && u->have_te[3], "unet: time_embed not loaded");
        float th[100];
        for (int k = 0; k < n_steps; ++k) th[k] = (float)sched.t[k];
        PD_HIP(hipMemcpyAsync(u->steps_t, th, n_steps * sizeof(float), hipMemcpyHostToDevice, s));
        PD_HIP(hipStreamSynchronize(s));         // `th` is a stack buffer
        PD_TRY(timestep_mlp(u->steps_t, n_steps, u->mc, u->te_w0, u->te_b0, u->te_w2, u->te_b2, u->steps_silu, u->steps_tmp, s));
        PD_TRY(gemv_rows(u->emb_w, u->emb_b, u->steps_silu, u->steps_emb, (int)u->emb_rows, u->ted, n_steps, s));
        u->steps_cached = n_steps;
    }
    const Tuning tun = tuning();
    for (int k = 0; k < n_steps; ++k) {
        PD_TRY(forward_impl(tun, u, u->sx, nullptr, N, u->set_, s, false, u->steps_emb + (size_t)k * u->emb_rows, 3));
        PD_TRY(ddnm_update(u->sx, u->set_, 3, u->sy, masks, eps_tape ? eps_tape + (size_t)k * n3 : nullptr, seed,
                           (unsigned long long)k + 1, sched.co[k], N, HW, s, quad0));
    }
    return ddnm_finish(u->sx, out, n3, s);
}
extern "C" int pdhip_ddnm_sample(pdhip_unet* u, const float* masked_imgs, const float* masks, int N, const float* x_T,
                                 const float* eps_tape, uint64_t seed, int n_steps, float* out, void* stream) {
    return pdhip_ddnm_sample_keyed(u, masked_imgs, masks, N, x_T, eps_tape, seed, 0, n_steps, out, stream);
}

// ---- the tuning / test hooks: every setter writes the calling thread's Tuning (csrc/nn_common.h lists the fields, their values and defaults)
// and returns the previous value of its (first) field
static int swap_hook(int& field, int v) { const int old = field; field = v; return old; }
extern "C" int pdhip_debug_set_conv_tile(int wmw) { return swap_hook(tuning().force_wmw, wmw); }
extern "C" int pdhip_debug_set_conv_stages(int st) { return swap_hook(tuning().force_stages, st); }
extern "C" int pdhip_debug_set_conv_bk(int bk) { return swap_hook(tuning().force_bk, bk); }
extern "C" int pdhip_debug_set_conv_halo_strips(int mode) { return swap_hook(tuning().halo_strips, mode); }
/* split-K workspace (device floats) for pdhip_conv2d_nhwc_f16 and a forced split factor (0 = automatic) */
extern "C" int pdhip_debug_set_conv_splitk(void* ws, long long ws_floats, int splits) {
    g_dbg_splitk_ws = (float*)ws; g_dbg_splitk_floats = ws ? (size_t)ws_floats : 0;
    if (ws != nullptr && ws_floats >= PD_SK_TICKET_FLOATS) (void)hipMemset(ws, 0, PD_SK_TICKET_FLOATS * sizeof(float));   // k_conv_sk's tickets start at zero
    return swap_hook(tuning().force_splits, splits);
}
extern "C" int pdhip_debug_set_conv_sk(int mode, int tile, int splits) { tuning().sk_tile = tile; tuning().sk_splits = splits; return swap_hook(tuning().sk_mode, mode); }
extern "C" int pdhip_debug_set_conv_sk_stages(int stages) { return swap_hook(tuning().sk_stages, stages); }
extern "C" int pdhip_debug_set_conv_sk_kgroups(int kg) { return swap_hook(tuning().sk_kg, kg); }
extern "C" int pdhip_debug_set_conv_sk_order(int order) { return swap_hook(tuning().sk_order, order); }
extern "C" int pdhip_debug_set_conv_rr(int mode, int variant, int slabs) { tuning().rr_variant = variant; tuning().rr_slabs = slabs; return swap_hook(tuning().rr_mode, mode); }
extern "C" int pdhip_debug_set_conv_ht(int mode, int slabs) { tuning().ht_slabs = slabs; return swap_hook(tuning().ht_mode, mode); }
extern "C" int pdhip_debug_set_fuse_gn(int on) { return swap_hook(tuning().fuse_gn, on); }
extern "C" int pdhip_debug_set_fold_resample(int on) { return swap_hook(tuning().fold_resample, on); }
extern "C" int pdhip_debug_set_fold_skip(int on) { return swap_hook(tuning().fold_skip, on); }
extern "C" int pdhip_debug_set_rr_gn(int max_width) { return swap_hook(tuning().rr_gn, max_width); }
extern "C" int pdhip_debug_set_fold_finalize(int max_batch) { return swap_hook(tuning().fold_finalize, max_batch); }
extern "C" int pdhip_debug_set_fold_finalize_chunks(int chunks) { return swap_hook(tuning().fold_finalize_chunks, chunks); }
extern "C" int pdhip_debug_set_fuse_skip(int mode, int min_tiles) { if (min_tiles > 0) tuning().fuse_skip_min_tiles = min_tiles; return swap_hook(tuning().fuse_skip, mode); }
extern "C" int pdhip_debug_set_up_phase(int mode) { return swap_hook(tuning().up_phase, mode); }
extern "C" int pdhip_debug_set_attn(int nbuf, int vt_form, int qtiles) {
    Tuning& t = tuning();
    const int old = t.attn_nbuf | (t.attn_vt << 8) | (t.attn_qtn << 16);
    t.attn_nbuf = nbuf; t.attn_vt = vt_form; t.attn_qtn = qtiles;
    return old;
}
extern "C" int pdhip_debug_set_gn_iters(int iters) { return swap_hook(tuning().gn_iters, iters); }
extern "C" int pdhip_debug_set_gn_skip_variant(int v) { return swap_hook(tuning().gs_variant, v); }

// ---- stand-alone operators (also the unit-test surface of the kernels)
extern "C" int pdhip_conv2d_nhwc_f16(const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                                     int N, int H, int W, int Cin, int Cout, int Cout_pad, int taps, const void* zero_page,
                                     void* stream) {
    PD_REQUIRE(x && w_packed && y && zero_page, "pdhip_conv2d_nhwc_f16: null argument");
    return conv_igemm(tuning(), (const half_t*)x, (const half_t*)w_packed, bias, (const half_t*)residual, (half_t*)y, N, H, W, Cin, Cout,
                      Cout_pad, taps, (const half_t*)zero_page, as_stream(stream), g_dbg_splitk_ws, g_dbg_splitk_floats);
}
/* test entry: conv_plan + conv_launch with every operand ConvArgs carries (include/pdhip.h).  What the planned kernel would drop silently is refused. */
extern "C" int pdhip_debug_conv_launch_nhwc_f16(const void* x, const void* x2, int Cin1, const void* w_packed, const float* bias, const void* residual,
                                                int res_up, const void* xs, const void* xs2, int Cs1, int Cs, void* y, int N, int H, int W, int Cin, int Cout,
                                                int Cout_pad, int taps, const void* zero_page, float* ws, long long ws_floats, float* gn_part,
                                                long long gn_part_floats, int* gn_chunks, int* kernel, void* stream) {
    const char* const fn = "pdhip_debug_conv_launch_nhwc_f16";
    PD_REQUIRE(x && w_packed && y && zero_page, "%s: null argument", fn);
    PD_REQUIRE(N > 0 && H > 0 && W > 0 && (taps == 1 || taps == 9), "%s: bad shape (N=%d H=%d W=%d taps=%d)", fn, N, H, W, taps);
    PD_REQUIRE(Cin % 32 == 0 && Cout % 8 == 0 && Cout_pad % 128 == 0 && Cout_pad >= Cout && Cin > 0 && Cout > 0,
               "%s: need Cin %% 32 == 0, Cout %% 8 == 0, padded Cout %% 128 == 0 (Cin=%d Cout=%d pad=%d)", fn, Cin, Cout, Cout_pad);
    PD_REQUIRE(x2 == nullptr || (taps == 1 && Cin1 > 0 && Cin1 < Cin && Cin1 % 64 == 0 && (Cin - Cin1) % 64 == 0),
               "%s: a two-source input needs a 1x1 conv and channel counts that are multiples of 64", fn);
    if (xs == nullptr) Cs = 0;
    PD_REQUIRE(xs == nullptr || (taps == 9 && Cs > 0 && Cs % 64 == 0 && (xs2 == nullptr || (Cs1 > 0 && Cs1 < Cs && Cs1 % 64 == 0))),
               "%s: a skip source needs a 3x3 conv and channel counts that are multiples of 64", fn);
    PD_REQUIRE(xs != nullptr || xs2 == nullptr, "%s: xs2 without xs", fn);
    PD_REQUIRE(xs == nullptr || residual == nullptr, "%s: the appended skip 1x1 takes the residual's place", fn);
    PD_REQUIRE(res_up == 0 || residual != nullptr, "%s: res_up without a residual", fn);
    const size_t wsf = ws != nullptr && ws_floats > 0 ? (size_t)ws_floats : 0;
    pdnn::ConvNeeds nd;
    nd.two_source = x2 != nullptr; nd.want_gn = gn_part != nullptr; nd.skip_cs = Cs;
    const pdnn::ConvPlan p = conv_plan(tuning(), N, H, W, Cin, Cout, Cout_pad, taps, nd, wsf);
    if (kernel) *kernel = (int)p.kernel;
    if (gn_chunks) *gn_chunks = p.gn_chunks;
    PD_REQUIRE(res_up == 0 || p.takes_res_up, "%s: the planned kernel (%s) does not read its residual at half resolution", fn, conv_kernel_name(p.kernel));
    PD_REQUIRE(Cs == 0 || p.takes_skip, "%s: the planned kernel (%s) does not append the skip 1x1", fn, conv_kernel_name(p.kernel));
    PD_REQUIRE(x2 == nullptr || p.kernel == pdnn::CONV_SK || p.kernel == pdnn::CONV_IGEMM, "%s: the planned kernel (%s) reads one source", fn,
               conv_kernel_name(p.kernel));
    PD_REQUIRE(gn_part == nullptr || gn_part_floats >= (long long)N * p.gn_chunks * (Cout / 8) * 2,
               "%s: gn_part holds %lld floats, the launch writes %lld", fn, gn_part_floats, (long long)N * p.gn_chunks * (Cout / 8) * 2);
    const pdnn::ConvArgs a{(const half_t*)x, (const half_t*)x2, x2 ? Cin1 : 0, (const half_t*)w_packed, bias, (const half_t*)residual, res_up, nullptr, nullptr,
                           (const half_t*)xs, (const half_t*)xs2, Cs1, (half_t*)y, (const half_t*)zero_page, wsf ? ws : nullptr, wsf, gn_part};
    return conv_launch(p, a, as_stream(stream));
}
extern "C" int pdhip_gn_finalize_oct_f32(const float* partA, int Ca, int chunksA, const float* partB, int Cb, int chunksB, int N, int HW, float* stats,
                                         void* stream) {
    PD_REQUIRE(partA && stats && N > 0 && HW > 0 && Ca > 0 && chunksA > 0, "pdhip_gn_finalize_oct_f32: bad arguments");
    PD_REQUIRE(partB ? (Cb > 0 && chunksB > 0) : Cb == 0, "pdhip_gn_finalize_oct_f32: partB and Cb / chunksB disagree");
    return gn_finalize_oct(partA, Ca, chunksA, partB, Cb, partB ? chunksB : 0, N, HW, 1e-5f, stats, as_stream(stream));
}
/* stand-alone: the packed 3x3 weights [Cout_pad][9 Cin] f16 -> phase weights [4][Cout_pad][4 Cin] f16 */
extern "C" int pdhip_pack_conv_up2_phase_f16(const void* w_packed, int Cin, int Cout_pad, void* w_phase, void* stream) {
    PD_REQUIRE(w_packed && w_phase && Cin > 0 && Cout_pad > 0, "pdhip_pack_conv_up2_phase_f16: bad arguments");
    return conv_up2_phase_pack((const half_t*)w_packed, Cin, Cout_pad, (half_t*)w_phase, as_stream(stream));
}
/* stand-alone: y [N,2H,2W,Cout] = conv3x3(nearest_x2(x [N,H,W,Cin])) + bias through the four phase convs; gn_part (may be NULL): GroupNorm octet
 * partials [N][4 H W / 256][Cout/8][2] */
extern "C" int pdhip_conv3x3_up2_phase_nhwc_f16(const void* x, const void* w_phase, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                                                int Cout_pad, const void* zero_page, float* gn_part, void* stream) {
    PD_REQUIRE(x && w_phase && y && zero_page, "pdhip_conv3x3_up2_phase_nhwc_f16: null argument");
    const pdnn::ConvPlan p = conv_up2_phase_plan(tuning(), N, 2 * H, 2 * W, Cin, Cout, Cout_pad, gn_part != nullptr);
    return conv_up2_phase((const half_t*)x, (const half_t*)w_phase, bias, (half_t*)y, N, H, W, Cin, Cout, Cout_pad, (const half_t*)zero_page,
                          as_stream(stream), p.gn_chunks > 0 ? gn_part : nullptr, p.geo);
}
/* stand-alone: the same layer on the 9-tap halo-resident kernel reading the half-resolution x with index arithmetic (the route the phase conv
 * replaces; layers that kernel takes unsplit only: 2W in {32 .. 256}) */
extern "C" int pdhip_conv3x3_up2_halo_nhwc_f16(const void* x, const void* w_packed, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                                               int Cout_pad, const void* zero_page, void* stream) {
    PD_REQUIRE(x && w_packed && y && zero_page, "pdhip_conv3x3_up2_halo_nhwc_f16: null argument");
    pdnn::ConvNeeds nd;
    nd.in_up = true;
    PD_REQUIRE(conv_plan(tuning(), N, 2 * H, 2 * W, Cin, Cout, Cout_pad, 9, nd, 0).takes_in_up,
               "pdhip_conv3x3_up2_halo_nhwc_f16: not a layer the halo-resident kernel takes unsplit");
    return conv_igemm(tuning(), (const half_t*)x, (const half_t*)w_packed, bias, nullptr, (half_t*)y, N, 2 * H, 2 * W, Cin, Cout, Cout_pad, 9,
                      (const half_t*)zero_page, as_stream(stream), nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 1);
}
/* stand-alone: h0 = silu(GroupNorm32(x)) and sk = conv1x1(x) (C -> 256) in one pass over x = [xa | xb] (xb NULL: single tensor, Ca == C);
 * stats [N][32][2] (mean, rstd) of x finished by the caller.  C % 256 == 0, Ca % 64 == 0, H * W % 128 == 0. */
extern "C" int pdhip_gn_silu_skip1x1_nhwc_f16(const void* xa, const void* xb, int Ca, int C, const float* stats, const float* gamma,
                                              const float* beta, const void* w_packed, const float* bias, void* h0, void* sk, int N, int H,
                                              int W, void* stream) {
    PD_REQUIRE(xa && stats && gamma && beta && w_packed && h0 && sk, "pdhip_gn_silu_skip1x1_nhwc_f16: null argument");
    return gn_skip((const half_t*)xa, (const half_t*)xb, Ca, C, stats, gamma, beta, (const half_t*)w_packed, bias, (half_t*)h0, (half_t*)sk,
                   N, H * W, as_stream(stream), tuning().gs_variant);
}
/* stand-alone: y = conv3x3( silu( GroupNorm32(x) [* (1 + scale) + shift] ) ) (+ residual) with the transform applied inside the
 * conv (halo-resident kernel; W in {32, 64, 128, 256}, H * W % 512 == 0, Cin % 32 == 0).  ws: N*64 + N*64*ceil(HW/256) + N*Cin*2 floats. */
extern "C" int pdhip_gn_silu_conv3x3_nhwc_f16(const void* x, const float* gamma, const float* beta, const float* film,
                                              long long film_stride, const void* w_packed, const float* bias, const void* residual,
                                              void* y, int N, int H, int W, int Cin, int Cout, int Cout_pad, const void* zero_page,
                                              float* ws, long long ws_floats, void* stream) {
    PD_REQUIRE(x && gamma && beta && w_packed && y && zero_page && ws, "pdhip_gn_silu_conv3x3_nhwc_f16: null argument");
    const size_t gws = (size_t)N * 64 * ((H * W + 255) / 256);
    PD_REQUIRE((size_t)ws_floats >= (size_t)N * 64 + gws + (size_t)N * Cin * 2, "pdhip_gn_silu_conv3x3_nhwc_f16: workspace too small");
    hipStream_t s = as_stream(stream);
    float* stats = ws;
    float* table = ws + (size_t)N * 64 + gws;
    PD_TRY(gn_stats((const half_t*)x, N, H * W, Cin, 1e-5f, stats, ws + (size_t)N * 64, gws, s));
    PD_TRY(gn_table(stats, gamma, beta, film, film_stride, N, Cin, table, s));
    // (the debug split-K workspace is shared with pdhip_conv2d_nhwc_f16, whose k_conv_sk route keeps its tickets in the first words)
    const pdnn::SplitWs sw = split_ws(g_dbg_splitk_ws, g_dbg_splitk_floats);
    float* const hws = sw.payload;
    const size_t hws_floats = sw.payload_floats;
    PD_REQUIRE(conv3x3_halo_eligible(N, H, W, Cin, Cout_pad) && N > 0 && Cout > 0 && Cout_pad > 0, "conv3x3_halo: unsupported geometry (N=%d H=%d W=%d Cin=%d)", N, H, W, Cin);
    return conv3x3_halo((const half_t*)x, (const half_t*)w_packed, bias, (const half_t*)residual, (half_t*)y, N, H, W, Cin, Cout,
                        Cout_pad, (const half_t*)zero_page, s, nullptr, conv3x3_halo_launch_splits(tuning(), N, H, W, Cin, Cout, Cout_pad, hws_floats),
                        conv3x3_halo_rows(tuning(), H, W), hws, hws_floats, table);
}
/* tuning hook: the APPLY conv on a ready-made (A, B) table [N][Cin/8][16] (tools/bench_conv.py --apply) */
extern "C" int pdhip_debug_conv3x3_apply(const void* x, const float* table, const void* w_packed, const float* bias, const void* residual,
                                         void* y, int N, int H, int W, int Cin, int Cout, int Cout_pad, const void* zero_page, void* stream) {
    PD_REQUIRE(x && table && w_packed && y && zero_page, "pdhip_debug_conv3x3_apply: null argument");
    return conv3x3_halo((const half_t*)x, (const half_t*)w_packed, bias, (const half_t*)residual, (half_t*)y, N, H, W, Cin, Cout,
                        Cout_pad, (const half_t*)zero_page, as_stream(stream), nullptr, 1, conv3x3_halo_rows(tuning(), H, W), nullptr, 0, table);
}
extern "C" int pdhip_pack_conv_weight_f16(const float* w_oihw, int Cout, int Cin, int taps, void* w_packed, void* stream) {
    PD_REQUIRE(w_oihw && w_packed, "pdhip_pack_conv_weight_f16: null argument");
    k_pack_conv<<<grid_for((long long)Cout * Cin * taps), 256, 0, as_stream(stream)>>>(w_oihw, 0, Cout, Cin, taps, (half_t*)w_packed);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
extern "C" int pdhip_groupnorm_nhwc_f16(const void* x, const float* gamma, const float* beta, const float* film, int N, int H,
                                        int W, int C, int silu, int resample, void* y, float* stats_ws /*[N*64]*/,
                                        float* ws, long long ws_floats, void* stream) {
    PD_REQUIRE(x && gamma && beta && y && stats_ws && ws, "pdhip_groupnorm_nhwc_f16: null argument");
    PD_TRY(gn_stats((const half_t*)x, N, H * W, C, 1e-5f, stats_ws, ws, (size_t)ws_floats, as_stream(stream)));
    return gn_apply((const half_t*)x, stats_ws, gamma, beta, film, 2LL * C, N, H, W, C, silu, resample, y, 0, as_stream(stream), nullptr, 0, nullptr, nullptr,
                    tuning().gn_iters);
}
// output head on its own: GroupNorm(32) statistics + the fused GN -> SiLU -> conv3x3 kernel (f32-equivalent arithmetic)
extern "C" size_t pdhip_unet_head_ws_floats(int N, int H, int W, int C, int Cout) {
    return (size_t)N * 64 + (size_t)N * 64 * ((H * W + 255) / 256) + (size_t)Cout * 9 * C + (size_t)64 * C;
}
extern "C" int pdhip_unet_head_f32(const void* x, const float* gamma, const float* beta, const float* w_oihw, const float* bias,
                                   int N, int H, int W, int C, int Cout, float* y_nchw, float* ws, long long ws_floats, void* stream) {
    PD_REQUIRE(x && gamma && beta && w_oihw && bias && y_nchw && ws, "pdhip_unet_head_f32: null argument");
    PD_REQUIRE((size_t)ws_floats >= pdhip_unet_head_ws_floats(N, H, W, C, Cout), "pdhip_unet_head_f32: workspace too small");
    hipStream_t s = as_stream(stream);
    float* stats = ws;
    float* gws = stats + (size_t)N * 64;
    const size_t gws_floats = (size_t)N * 64 * ((H * W + 255) / 256);
    float* wp = gws + gws_floats;
    half_t* wz = reinterpret_cast<half_t*>(wp + (size_t)Cout * 9 * C);
    PD_TRY(gn_stats((const half_t*)x, N, H * W, C, 1e-5f, stats, gws, gws_floats, s));
    k_pack_conv_f32<<<grid_for((long long)Cout * 9 * C), 256, 0, s>>>(w_oihw, 0, Cout, C, 9, wp);
    PD_LAUNCH_CHECK();
    PD_TRY(head_pack(wp, Cout, C, wz, s));
    return head_gn_silu_conv3x3((const half_t*)x, stats, gamma, beta, wz, bias, y_nchw, N, H, W, C, Cout, s);
}
extern "C" int pdhip_attention_f16(const void* qkv, void* out, int N, int T, int C, int head_dim, void* vt_ws, void* stream) {
    PD_REQUIRE(qkv && out, "pdhip_attention_f16: null argument");
    const Tuning& t = tuning();
    return attention((const half_t*)qkv, (half_t*)out, N, T, C, head_dim, as_stream(stream), (half_t*)vt_ws, t.attn_nbuf, t.attn_qtn, t.attn_vt);
}
extern "C" int pdhip_philox_normal(float* out, long long n, uint64_t seed, uint64_t stream_id, void* stream) {
    PD_REQUIRE(out && n > 0, "pdhip_philox_normal: bad arguments");
    return philox_normal(out, n, seed, stream_id, as_stream(stream));
}
extern "C" int pdhip_bench_copy16(const void* src, void* dst, long long bytes, int blocks, int unroll, void* stream) {
    return copy16(src, dst, bytes, blocks, unroll, as_stream(stream));
}
// ---- the GroupNorm-apply pass and its neighbours on their own (csrc/nn_norm.hip): unit-test surface, nothing the product calls
extern "C" int pdhip_gn_apply_f16(const void* x, const void* x2, int Ca, int C, const float* stats, const float* partA, int chunksA,
                                  const float* partB, int chunksB, const float* gamma, const float* beta, const float* film,
                                  long long film_stride, int N, int H, int W, int silu, int resample, void* y, void* y_raw, void* stream) {
    PD_REQUIRE(x && gamma && beta && y, "pdhip_gn_apply_f16: null argument");
    PD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "pdhip_gn_apply_f16: empty tensor");
    PD_REQUIRE((stats != nullptr) != (partA != nullptr), "pdhip_gn_apply_f16: the statistics come finished (stats) or as octet partials (partA), not both");
    PD_REQUIRE(stats == nullptr || (partB == nullptr && chunksA == 0 && chunksB == 0), "pdhip_gn_apply_f16: partials next to finished statistics");
    PD_REQUIRE(partA == nullptr || (chunksA >= 1 && (x2 == nullptr ? (partB == nullptr && chunksB == 0) : (partB != nullptr && chunksB >= 1))),
               "pdhip_gn_apply_f16: one set of octet partials (and a chunk count >= 1) per source tensor");
    PD_REQUIRE(film == nullptr || film_stride >= 2LL * C, "pdhip_gn_apply_f16: film rows hold scale[C] | shift[C]");
    if (partA != nullptr) {
        const GnPartsArg pa{partA, x2 ? Ca : C, chunksA, partB, x2 ? C - Ca : 0, chunksB, 1e-5f};
        return gn_apply((const half_t*)x, nullptr, gamma, beta, film, film_stride, N, H, W, C, silu, resample, y, 0, as_stream(stream),
                        (const half_t*)x2, x2 ? Ca : 0, (half_t*)y_raw, &pa, tuning().gn_iters);
    }
    return gn_apply((const half_t*)x, stats, gamma, beta, film, film_stride, N, H, W, C, silu, resample, y, 0, as_stream(stream),
                    (const half_t*)x2, x2 ? Ca : 0, (half_t*)y_raw, nullptr, tuning().gn_iters);
}
extern "C" int pdhip_gn_table_f32(const float* stats, const float* gamma, const float* beta, const float* film, long long film_stride, int N, int C,
                                  float* table, void* stream) {
    PD_REQUIRE(stats && gamma && beta && table && N > 0 && C > 0, "pdhip_gn_table_f32: bad arguments");
    PD_REQUIRE(film == nullptr || film_stride >= 2LL * C, "pdhip_gn_table_f32: film rows hold scale[C] | shift[C]");
    return gn_table(stats, gamma, beta, film, film_stride, N, C, table, as_stream(stream));
}
extern "C" int pdhip_resample2x_nhwc_f16(const void* x, int N, int H, int W, int C, int mode, void* y, void* stream) {
    PD_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0, "pdhip_resample2x_nhwc_f16: bad arguments");
    PD_REQUIRE(mode != 1 || (H % 2 == 0 && W % 2 == 0), "pdhip_resample2x_nhwc_f16: avgpool needs even H, W");
    return resample2x((const half_t*)x, N, H, W, C, mode, (half_t*)y, as_stream(stream));
}
extern "C" int pdhip_concat_channels_f16(const void* a, int Ca, const void* b, int Cb, long long pixels, void* y, void* stream) {
    PD_REQUIRE(a && b && y && Ca > 0 && Cb > 0 && pixels > 0, "pdhip_concat_channels_f16: bad arguments");
    return concat_channels((const half_t*)a, Ca, (const half_t*)b, Cb, pixels, (half_t*)y, as_stream(stream));
}
