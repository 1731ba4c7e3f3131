// P25 channel front (capture.py:2619-2700) for gfx950: freq_shift (capture.py:166-193) then decimate_iq_for_p25
// (capture.py:203-295), for n_channels live P25 channels that share one wideband complex64 chunk.
//   * subsample / pass-through plan: one kernel, out[j] = x[j D] * exp(i c f32(j D)); the NCO phase is evaluated at the
//     kept samples only (the reference mixes every sample and then slices [::D]; the kept values are the same).
//   * resample plan (scipy.signal.resample_poly, up / down): one workgroup per 64 kept outputs of one channel.  It mixes
//     the input span those outputs reach into LDS once (stored phase-major, see the kernel), then each lane runs one
//     output's dot product for both rails.  scipy casts the taps to the input's dtype (float32) and upfirdn accumulates
//     in float32, oldest sample first, one rounded product and one rounded add per tap: the loop repeats that order
//     with __fmul_rn / __fadd_rn, so no product is contracted into an FMA.
// Offsets and the active set travel in the launch arguments (up to P25F_LAUNCH_CHANNELS channels per launch): the
// handle owns the taps and nothing else, so nothing grows and no call synchronises.
#include "wh_common.h"
#include "wh_portable_math.h"
#include <cmath>
#include <memory>
#include <numeric>
#include <vector>

using namespace wh;

namespace {

constexpr int P25F_TARGET_RATE = 48000;      // decimate_iq_for_p25's TARGET_RATE
constexpr int P25F_SUBSAMPLE_ABOVE = 50;     // `down > 50` -> plain subsampling
constexpr int P25F_LAUNCH_CHANNELS = 64;     // channels per launch (kernel arguments)
constexpr int P25F_OPW = 64;                 // resample plan: kept outputs per workgroup (one wave, one per lane)
constexpr int P25F_FILL = 8;                 // resample plan: input loads in flight per lane while the tile fills
constexpr size_t P25F_MAX_N = (size_t)1 << 24;   // the float32 sample index is exact up to here

struct P25fArgs {
    const float2 *x;
    float2 *out;
    size_t out_stride;
    int n, m;                       // input samples, kept outputs per channel
    int step;                       // subsample: D (1 = pass-through); resample: down
    int up, L, pre_pad, imax;       // resample only: phase count, taps, scipy's n_pre_pad, max tap-row index
    long long P0;                   // resample only: n_pre_remove * down (first kept output's upsampled position)
    int tile_r;                     // tile rows (down when up == 1, else 1)
    int tile_w;                     // tile row length
    const float *taps;              // [L] float32
    int row[P25F_LAUNCH_CHANNELS];  // output row of launch slot y
    float c[P25F_LAUNCH_CHANNELS];  // f32(-2 pi round(off)/fs); 0 = no mix (freq_shift returns its input)
};

// freq_shift's sample: x[s] * complex64(exp(i * f32(c) * f32(s))).  numpy's complex64 product is the fused
// multiply-add/subtract form (re = fma(a.re, b.re, -(a.im b.im)), im = fma(a.re, b.im, a.im b.re)).
__device__ __forceinline__ float2 p25f_mix(float2 v, float c, int s) {
    if (c == 0.0f) return v;
    float ph = __fmul_rn(c, (float)s);
    float sn, cs;
    whm_sincos_phase(ph, &sn, &cs);
    return make_float2(fmaf(v.x, cs, -__fmul_rn(v.y, sn)), fmaf(v.x, sn, __fmul_rn(v.y, cs)));
}

__global__ __launch_bounds__(256) void p25f_subsample_kernel(P25fArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    const int s = j * a.step;
    a.out[(size_t)a.row[blockIdx.y] * a.out_stride + j] = p25f_mix(a.x[s], a.c[blockIdx.y], s);
}

// The tile holds the span phase-major: sample k at (k % tile_r) * tile_w + k / tile_r.  With up == 1 lane o of a wave
// reads sample o*down + const for each tap, so with tile_r = down the wave's 64 reads of one tap are 64 consecutive
// float2 (ds_read_b64, no bank conflict).  With up > 1, tile_r = 1 (the plain order).

// y[m] = sum_i x[q0 - i] * h[i up + t - pre_pad], P = P0 + m down, q0 = P / up, t = P % up; i descending (oldest
// sample first), taps outside [0, L) and samples outside [0, n) contribute nothing (zero padding).
__global__ __launch_bounds__(P25F_OPW) void p25f_resample_kernel(P25fArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    float *tp = reinterpret_cast<float *>(sm_raw);
    float2 *tile = reinterpret_cast<float2 *>(sm_raw + (((size_t)a.L * sizeof(float) + 15) & ~(size_t)15));
    const int o = threadIdx.x;
    const int m0 = blockIdx.x * P25F_OPW;
    const int mc = min(P25F_OPW, a.m - m0);
    const float c = a.c[blockIdx.y];
    const long long q_first = (a.P0 + (long long)m0 * a.step) / a.up;
    const long long q_last = (a.P0 + (long long)(m0 + mc - 1) * a.step) / a.up;
    const long long lo = q_first - a.imax;          // oldest sample any output of this workgroup reaches
    const int span = (int)(q_last - lo + 1);
    for (int i = o; i < a.L; i += P25F_OPW) tp[i] = a.taps[i];
    // fill: P25F_FILL loads in flight per lane before any is mixed (one wave per SIMD cannot hide a load's latency
    // otherwise); the tile position of k = o + 64 j advances by 64 % tile_r rows and 64 / tile_r columns per step
    const int dr = P25F_OPW % a.tile_r, dc = P25F_OPW / a.tile_r;
    int fr = o % a.tile_r, fc = o / a.tile_r;
    for (int kb = o; kb < span; kb += P25F_OPW * P25F_FILL) {
        float2 v[P25F_FILL];
#pragma unroll
        for (int u = 0; u < P25F_FILL; ++u) {
            const long long s = lo + kb + u * P25F_OPW;
            v[u] = (kb + u * P25F_OPW < span && s >= 0 && s < a.n) ? a.x[s] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < P25F_FILL; ++u) {
            const int k = kb + u * P25F_OPW;
            const long long s = lo + k;
            if (k < span) tile[fr * a.tile_w + fc] = (s >= 0 && s < a.n) ? p25f_mix(v[u], c, (int)s) : v[u];
            fr += dr;
            fc += dc;
            if (fr >= a.tile_r) { fr -= a.tile_r; ++fc; }
        }
    }
    __syncthreads();
    if (o >= mc) return;
    const long long P = a.P0 + (long long)(m0 + o) * a.step;
    const int q0 = (int)(P / a.up - lo);            // q0 in span coordinates
    const int t = (int)(P % a.up);
    // taps: 0 <= i up + t - pre_pad <= L - 1
    const int i_lo = max(0, (a.pre_pad - t + a.up - 1) / a.up);
    const int i_hi = (a.L - 1 + a.pre_pad - t) / a.up;
    // walk oldest sample -> newest: the tap index falls by up, the span index rises by one
    const int k0 = q0 - i_hi;
    int left = i_hi - i_lo + 1;
    int hi = i_hi * a.up + t - a.pre_pad;
    float ar = 0.0f, ai = 0.0f;
    if (a.tile_r == 1) {                            // up > 1: plain tile
        for (int k = k0; left > 0; ++k, --left, hi -= a.up) {
            const float h = tp[hi];
            const float2 v = tile[k];
            ar = __fadd_rn(ar, __fmul_rn(v.x, h));
            ai = __fadd_rn(ai, __fmul_rn(v.y, h));
        }
    } else {
        // up == 1: every lane starts in the same tile row r (k0 = o down + const), so the runs along a column of the
        // phase-major tile are the same length in every lane; each run's loads do not depend on the sums and unroll
        int r = k0 % a.tile_r, c = k0 / a.tile_r;
        while (left > 0) {
            const int run = min(a.tile_r - r, left);
            const float2 *col = tile + r * a.tile_w + c;
            const float *h = tp + hi;
#pragma unroll 8
            for (int u = 0; u < run; ++u) {
                const float2 v = col[u * a.tile_w];
                const float w = h[-u];
                ar = __fadd_rn(ar, __fmul_rn(v.x, w));
                ai = __fadd_rn(ai, __fmul_rn(v.y, w));
            }
            hi -= run;
            left -= run;
            r = 0;
            ++c;
        }
    }
    a.out[(size_t)a.row[blockIdx.y] * a.out_stride + m0 + o] = make_float2(ar, ai);
}

}  // namespace

struct wh_p25front {
    int C, fs;
    int resample;                 // 0: subsample / pass-through, 1: resample_poly
    int step, up, L, pre_pad, imax, n_pre_remove;
    std::vector<float> c;         // per channel NCO constant (0 = no mix)
    DevBuf<float> d_taps;
};

extern "C" int wh_p25front_create(wh_p25front **out, int n_channels, int sample_rate, const float *h_taps, int ntaps) {
    if (!out || n_channels < 1 || sample_rate < 1) return set_err(WH_E_ARG, "wh_p25front_create: bad arguments");
    std::unique_ptr<wh_p25front> f(new wh_p25front());   // frees partial state on early return
    f->C = n_channels;
    f->fs = sample_rate;
    f->c.assign((size_t)n_channels, 0.0f);
    f->step = 1; f->up = 1; f->L = 0; f->pre_pad = 0; f->imax = 0; f->n_pre_remove = 0;
    f->resample = 0;
    if (sample_rate > P25F_TARGET_RATE) {
        const int g = std::gcd(sample_rate, P25F_TARGET_RATE);
        const int up = P25F_TARGET_RATE / g, down = sample_rate / g;
        if (down > P25F_SUBSAMPLE_ABOVE) {
            f->step = sample_rate / P25F_TARGET_RATE;
        } else {
            const int half_len = 10 * (up > down ? up : down);
            if (!h_taps || ntaps != 2 * half_len + 1)
                return set_err(WH_E_ARG, "wh_p25front_create: rate %d resamples %d/%d and needs the %d resample_poly taps",
                               sample_rate, up, down, 2 * half_len + 1);
            f->resample = 1;
            f->step = down;
            f->up = up;
            f->L = ntaps;
            f->pre_pad = down - half_len % down;                 // scipy's n_pre_pad
            f->n_pre_remove = (half_len + f->pre_pad) / down;    // scipy's n_pre_remove
            f->imax = (ntaps - 1 + f->pre_pad) / up;
            WH_HIP(f->d_taps.alloc((size_t)ntaps));
            WH_HIP(hipMemcpy(f->d_taps, h_taps, (size_t)ntaps * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    *out = f.release();
    return WH_OK;
}

extern "C" void wh_p25front_destroy(wh_p25front *f) { delete f; }

extern "C" int wh_p25front_set_offsets(wh_p25front *f, const double *h_offsets_hz) {
    if (!f || !h_offsets_hz) return set_err(WH_E_ARG, "wh_p25front_set_offsets: null argument");
    for (int k = 0; k < f->C; ++k)
        if (!std::isfinite(h_offsets_hz[k]) || std::fabs(h_offsets_hz[k]) > 1e9)
            return set_err(WH_E_ARG, "wh_p25front_set_offsets: offset %d is not a finite value within 1e9 Hz", k);
    for (int k = 0; k < f->C; ++k) {
        const double r = std::nearbyint(h_offsets_hz[k]);    // Python round(): half to even (default rounding mode)
        // f32(-2 pi (round(off)/fs)): the Python complex scalar is weak -> cast to complex64 (capture.py:173-176)
        f->c[k] = r == 0.0 ? 0.0f : (float)(-2.0 * M_PI * (r / (double)f->fs));
    }
    return WH_OK;
}

static size_t p25f_out_len(const wh_p25front *f, size_t n) {
    if (f->resample) {
        const size_t nu = n * (size_t)f->up;
        return nu / (size_t)f->step + (nu % (size_t)f->step ? 1 : 0);
    }
    return (n + (size_t)f->step - 1) / (size_t)f->step;
}

extern "C" size_t wh_p25front_out_len(const wh_p25front *f, size_t n) { return f ? p25f_out_len(f, n) : 0; }

extern "C" int wh_p25front_run(wh_p25front *f, const float *d_iq, size_t n, const unsigned char *h_active, float *d_out,
                               size_t out_stride, void *stream) {
    if (!f) return set_err(WH_E_ARG, "wh_p25front_run: null handle");
    if (n > P25F_MAX_N) return set_err(WH_E_ARG, "wh_p25front_run: n > 2^24 (float32 sample index is not exact beyond)");
    if (n == 0) return WH_OK;
    if (!d_iq || !d_out) return set_err(WH_E_ARG, "wh_p25front_run: null buffer");
    const size_t m = p25f_out_len(f, n);
    if (out_stride < m) return set_err(WH_E_ARG, "wh_p25front_run: out_stride %zu < out_len %zu", out_stride, m);
    hipStream_t st = as_stream(stream);
    P25fArgs a{};
    a.x = reinterpret_cast<const float2 *>(d_iq);
    a.out = reinterpret_cast<float2 *>(d_out);
    a.out_stride = out_stride;
    a.n = (int)n;
    a.m = (int)m;
    a.step = f->step;
    a.up = f->up;
    a.L = f->L;
    a.pre_pad = f->pre_pad;
    a.imax = f->imax;
    a.P0 = (long long)f->n_pre_remove * f->step;
    a.taps = f->d_taps;
    size_t smem = 0;
    if (f->resample) {
        a.tile_r = f->up == 1 ? f->step : 1;
        // span of one workgroup: q_last - q_first + imax + 1, q_last - q_first <= ((OPW - 1) down) / up + 1
        const int span_max = ((P25F_OPW - 1) * f->step) / f->up + 2 + f->imax;
        a.tile_w = (span_max + a.tile_r - 1) / a.tile_r;
        smem = (((size_t)f->L * sizeof(float) + 15) & ~(size_t)15) + (size_t)a.tile_r * a.tile_w * sizeof(float2);
    }
    int k = 0;
    while (k < f->C) {
        int cnt = 0;
        for (; k < f->C && cnt < P25F_LAUNCH_CHANNELS; ++k) {
            if (h_active && !h_active[k]) continue;
            a.row[cnt] = k;
            a.c[cnt] = f->c[(size_t)k];
            ++cnt;
        }
        if (cnt == 0) break;
        if (f->resample) {
            hipLaunchKernelGGL(p25f_resample_kernel, dim3((unsigned)((m + P25F_OPW - 1) / P25F_OPW), (unsigned)cnt),
                               dim3(P25F_OPW), smem, st, a);
        } else {
            hipLaunchKernelGGL(p25f_subsample_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)cnt), dim3(256), 0,
                               st, a);
        }
        WH_LAUNCH_CHECK();
    }
    return WH_OK;
}
