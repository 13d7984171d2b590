// Image metrics of the evaluation path (utils/metric_utils/psnr_ssmi.py): per image of two u8 batches [N,H,W,C] the exact integer
// sum of squared differences (PSNR is computed from it on the host) and the mean SSIM in float64, in one of two definitions:
//   uniform  : skimage.metrics.structural_similarity(data_range=255, channel_axis=2) -- 7x7 uniform window, sample covariance
//              (49/48), mean over the image with a 3-pixel border cropped, i.e. over the windows that lie inside the image;
//   gaussian : psnr_ssmi.py:127-147 -- outer product of an 11-tap Gaussian (sigma 1.5, sum 1), "valid" region, population covariance.
// Both with C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.  A workgroup stages a 32 x 16 output tile plus its halo of both images (all
// channels) in LDS, filters it separably (rows, then columns), and reduces its S values in a fixed order; a second kernel adds the
// workgroup partials of an image in a fixed order.  No floating-point atomics: two runs give equal bits.
#include "common.h"
#include <math.h>
#include <type_traits>

namespace pdhip {

constexpr int MT_X = 32, MT_Y = 16, MT_MAXC = 4;
struct GaussTaps { double g[11]; };

template <int WIN, bool GAUSS>
__global__ __launch_bounds__(256) void k_image_metrics(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W, int C,
                                                       int do_ssim, GaussTaps gw, double* __restrict__ part_ssim,
                                                       unsigned long long* __restrict__ part_sse) {
    constexpr int HX = MT_X + WIN - 1, HY = MT_Y + WIN - 1;
    using T = typename std::conditional<GAUSS, double, int>::type;
    __shared__ uint8_t sa[HY * HX * MT_MAXC], sb[HY * HX * MT_MAXC];
    __shared__ T hs[5][HY][MT_X];
    __shared__ double red_s[4];
    __shared__ unsigned long long red_e[4];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * MT_X, ty0 = blockIdx.y * MT_Y;
    const size_t img = (size_t)blockIdx.z * H * W * C;
    const uint8_t* A = a + img;
    const uint8_t* B = b + img;
    const int rowbytes = HX * C, imgrow = W * C;
    unsigned int sse = 0;                                         // <= 8 elements per thread, 65025 each
    for (int e = tid; e < HY * rowbytes; e += 256) {
        const int r = e / rowbytes, q = e - r * rowbytes;
        const int y = ty0 + r, xb = tx0 * C + q;
        int va = 0, vb = 0;
        if (y < H && xb < imgrow) {
            va = A[(size_t)y * imgrow + xb];
            vb = B[(size_t)y * imgrow + xb];
            if (r < MT_Y && q < MT_X * C) sse += (unsigned)((va - vb) * (va - vb));     // the tile's own pixels: every pixel once
        }
        sa[e] = (uint8_t)va;
        sb[e] = (uint8_t)vb;
    }
    __syncthreads();
    const int outH = H - WIN + 1, outW = W - WIN + 1;
    double acc = 0.0;
    if (do_ssim) {
        for (int c = 0; c < C; ++c) {
            for (int e = tid; e < HY * MT_X; e += 256) {          // rows: WIN taps along x
                const int r = e / MT_X, x = e - r * MT_X;
                T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
                for (int k = 0; k < WIN; ++k) {
                    const int va = sa[r * rowbytes + (x + k) * C + c], vb = sb[r * rowbytes + (x + k) * C + c];
                    if (GAUSS) {
                        const double g = gw.g[k];
                        s0 += g * (double)va; s1 += g * (double)vb;
                        s2 += g * (double)(va * va); s3 += g * (double)(vb * vb); s4 += g * (double)(va * vb);
                    } else {
                        s0 += va; s1 += vb; s2 += va * va; s3 += vb * vb; s4 += va * vb;
                    }
                }
                hs[0][r][x] = s0; hs[1][r][x] = s1; hs[2][r][x] = s2; hs[3][r][x] = s3; hs[4][r][x] = s4;
            }
            __syncthreads();
            for (int e = tid; e < MT_Y * MT_X; e += 256) {        // columns: WIN taps along y, then S of the window
                const int y = e / MT_X, x = e - y * MT_X;
                if (ty0 + y < outH && tx0 + x < outW) {
                    T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        if (GAUSS) {
                            const double g = gw.g[k];
                            s0 += g * hs[0][y + k][x]; s1 += g * hs[1][y + k][x]; s2 += g * hs[2][y + k][x];
                            s3 += g * hs[3][y + k][x]; s4 += g * hs[4][y + k][x];
                        } else {
                            s0 += hs[0][y + k][x]; s1 += hs[1][y + k][x]; s2 += hs[2][y + k][x];
                            s3 += hs[3][y + k][x]; s4 += hs[4][y + k][x];
                        }
                    }
                    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
                    double ux, uy, vx, vy, vxy;
                    if (GAUSS) {
                        ux = (double)s0; uy = (double)s1;
                        vx = (double)s2 - ux * ux; vy = (double)s3 - uy * uy; vxy = (double)s4 - ux * uy;
                    } else {
                        // window sums are exact integers (<= 49 * 255^2): n * sum(x^2) - sum(x)^2 is the exact n^2-fold population variance
                        constexpr long long NP = (long long)WIN * WIN;
                        const long long ix = (long long)s0, iy = (long long)s1;
                        ux = (double)ix / (double)NP; uy = (double)iy / (double)NP;
                        const double norm = (double)(NP * (NP - 1));
                        vx = (double)(NP * (long long)s2 - ix * ix) / norm;
                        vy = (double)(NP * (long long)s3 - iy * iy) / norm;
                        vxy = (double)(NP * (long long)s4 - ix * iy) / norm;
                    }
                    acc += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
                }
            }
            __syncthreads();
        }
    }
    // fixed-order reduction: butterfly inside the wave, then the four waves in order
    unsigned long long e64 = sse;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        e64 += __shfl_down(e64, off, 64);
    }
    if ((tid & 63) == 0) { red_s[tid >> 6] = acc; red_e[tid >> 6] = e64; }
    __syncthreads();
    if (tid == 0) {
        const size_t p = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part_ssim[p] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        part_sse[p] = red_e[0] + red_e[1] + red_e[2] + red_e[3];
    }
}

__global__ __launch_bounds__(256) void k_image_metrics_finalize(const double* __restrict__ part_ssim,
                                                                const unsigned long long* __restrict__ part_sse, int nblk, double count,
                                                                unsigned long long* __restrict__ sse, double* __restrict__ ssim) {
    __shared__ double rs[256];
    __shared__ unsigned long long re[256];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nblk;
    double s = 0.0;
    unsigned long long e = 0;
    for (int i = tid; i < nblk; i += 256) { s += part_ssim[base + i]; e += part_sse[base + i]; }
    rs[tid] = s; re[tid] = e;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { rs[tid] += rs[tid + off]; re[tid] += re[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (sse) sse[blockIdx.x] = re[0];
        if (ssim) ssim[blockIdx.x] = rs[0] / count;
    }
}

static inline long long metrics_blocks(int H, int W) { return (long long)cdiv(H, MT_Y) * cdiv(W, MT_X); }

}  // namespace pdhip

using namespace pdhip;

extern "C" size_t pdhip_image_metrics_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    Carve cv{nullptr, 0};
    cv.take<double>((size_t)N * metrics_blocks(H, W));
    cv.take<unsigned long long>((size_t)N * metrics_blocks(H, W));
    return cv.bytes();
}

extern "C" int pdhip_image_metrics(const uint8_t* a, const uint8_t* b, int N, int H, int W, int C, int gaussian, uint64_t* sse,
                                   double* ssim, void* ws, void* stream) {
    PD_REQUIRE(a && b && ws, "pdhip_image_metrics: a, b and ws must not be NULL");
    PD_REQUIRE(sse || ssim, "pdhip_image_metrics: sse and ssim are both NULL");
    PD_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768,
               "pdhip_image_metrics: N = %d (1 .. 65535), H = %d, W = %d (1 .. 32768)", N, H, W);
    PD_REQUIRE(C >= 1 && C <= MT_MAXC, "pdhip_image_metrics: C = %d channels (1 .. %d)", C, MT_MAXC);
    PD_REQUIRE(gaussian == 0 || gaussian == 1, "pdhip_image_metrics: gaussian = %d (0 = 7x7 uniform window, 1 = 11x11 Gaussian)", gaussian);
    const int win = gaussian ? 11 : 7;
    PD_REQUIRE(!ssim || (H >= win && W >= win), "pdhip_image_metrics: a %d x %d image is smaller than the %d x %d SSIM window", H, W, win, win);
    const long long nblk = metrics_blocks(H, W);
    Carve cv{reinterpret_cast<char*>(ws), 0};
    double* part_ssim = cv.take<double>((size_t)N * nblk);
    unsigned long long* part_sse = cv.take<unsigned long long>((size_t)N * nblk);
    GaussTaps gw;
    double sum = 0.0;
    for (int k = 0; k < 11; ++k) { gw.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += gw.g[k]; }
    for (int k = 0; k < 11; ++k) gw.g[k] /= sum;
    const dim3 grid(cdiv(W, MT_X), cdiv(H, MT_Y), N);
    if (gaussian)
        k_image_metrics<11, true><<<grid, 256, 0, as_stream(stream)>>>(a, b, H, W, C, ssim != nullptr, gw, part_ssim, part_sse);
    else
        k_image_metrics<7, false><<<grid, 256, 0, as_stream(stream)>>>(a, b, H, W, C, ssim != nullptr, gw, part_ssim, part_sse);
    PD_LAUNCH_CHECK();
    const double count = ssim ? (double)(H - win + 1) * (double)(W - win + 1) * C : 1.0;
    k_image_metrics_finalize<<<N, 256, 0, as_stream(stream)>>>(part_ssim, part_sse, (int)nblk, count,
                                                               reinterpret_cast<unsigned long long*>(sse), ssim);
    PD_LAUNCH_CHECK();
    return PDHIP_OK;
}
