// Voice-recorder symbol path for gfx950: the FM discriminator of VoiceRecorder.process_iq (trunking/system.py:708-717)
// and the reference's DiscriminatorDemodulator (decoders/p25.py:1105-1345) as a bank of C independent channels.  One
// run() per channel is exactly ONE demodulate() call of the reference: the auto-gain is per call and the 'same'-mode
// low-pass re-seeds on every call, so the result depends on where a stream is cut and a call is never split.
//   k_disc_angle  (run_iq only) thread per sample: float64 angle of the decimated IQ and np.unwrap's per-sample
//                 correction ph_correct (numpy 2.2 unwrap: mod(dd + pi, 2 pi) - pi, +pi on the ambiguous boundary,
//                 0 where |dd| < pi), the first difference taken against the carried UNWRAPPED last phase;
//   k_disc_prep   ONE WAVE PER CHANNEL: finiteness gate of the row, then (run_iq) the sequential float64 cumsum of the
//                 corrections -> unwrapped phase -> first difference -> float32 disc audio, then the per-call auto-gain
//                 (p25.py:1218-1227) and the per-sample DC tracker (:1229-1235) -- 64 samples are loaded by the 64
//                 lanes, and every lane runs the same uniform loop over them through v_readlane;
//   k_disc_lpf    thread per sample: the 65-tap Hamming low-pass, np.convolve(..., 'same'), only when len >= 65,
//                 accumulated in float64 and rounded to float32 (numpy's own float32 convolve goes through sdot, whose
//                 summation order is the BLAS's; tools/gen_golden_voice.py keeps only cases whose dibits do not move
//                 under that difference);
//   k_disc_sym    ONE WAVE PER CHANNEL: _mmse_timing_recovery (:1255-1333) -- symbol clock, two 8-tap MMSE
//                 interpolations per symbol from a 128-entry LDS window of the filtered samples, the spread / timing /
//                 fine / coarse loops and the 4-level slicer; the 8-sample history and its index are carried.
//
// Scalar types.  The reference mixes Python floats (float64) and np.float32 scalars under NumPy-2 (NEP 50) promotion: a
// Python float meeting a float32 is cast to float32 first, comparisons included, and Python's min / max return
// whichever operand they pick, with its type.  Every state variable therefore carries an "is float32" flag:
//   variable      starts as         becomes float32                                  back to float64
//   input_gain    1.0 (float64)     at the first auto-gain update:                   never (reset() keeps it)
//                                   g*0.9 [f64 product cast, or f32] + f32(3/max)*0.1f
//   dc_estimate   0.0 (float64)     at the first sample: (f32)(dc*0.999) + s*0.001f  reset()
//   symbol_clock  0.0 (float64)     at the first symbol's timing update               reset()
//                                   (before it: += 0.1 and -= 1.0 in float64)
//   fine_freq     0.0 (float64)     at the first symbol: f32(fine) + e*0.125f        reset()
//   coarse_freq   0.0 (float64)     at the SECOND symbol: at the first one fine and coarse are both Python floats, so
//                                   coarse += (fine - coarse)*K stays float64 (0.0)  reset()
//   symbol_spread 2.0 (float64)     at every spread update (f32(spread) -/+ e*...)   whenever max(1.6, min(2.4, s))
//                                                                                    clamps: the literal 2.4 / 1.6
//   mu            float64 while the clock is float64, float32 after; min(mu, 1.0) returns the Python 1.0 when it clamps
//   interp        float32: sum from 0.0 of separately rounded f32 products, in tap order; then -= f32(fine)
//   symbol_error  float32: interp +- (1.5 | 0.5) * spread, the product in float64 when spread is a Python float
//   output        float32: (2 * interp) / f32(spread)
// round(mu * 128) rounds half to even (rint) in the type of mu; the product is exact either way.  Every float32
// operation is an explicit __f*_rn (no FMA contraction), every float64 one an explicit __d*_rn.
#include "wh_common.h"
#include <cmath>
#include <memory>
#include <vector>

using namespace wh;

namespace {

constexpr int NT = 8;          // MMSE_NTAPS (p25.py:1122)
constexpr int NSTEPS = 128;    // MMSE_NSTEPS
constexpr int MAX_BB = 255;    // longest baseband filter the LDS tile takes (the reference's is 65)
constexpr int TILE = 256;
constexpr double PI_D = 3.141592653589793;

struct DiscState {
    double clock, spread, dc, fine, coarse, gain;  // a float32 value is held exactly in the double
    double last_phase;                              // carried UNWRAPPED phase (system.py:715)
    long long symbol_count;
    float hist[NT];                                 // filtered history, oldest first
    int clock_f, spread_f, dc_f, fine_f, coarse_f, gain_f;
    int hist_idx;                                   // the reference's _history_idx (ring position of the oldest)
    int pad;
};

constexpr int MASK_WORDS = WH_DISC_MAX_CHANNELS / 32;

struct DiscArgs {
    const float *audio;    // [C][stride] float32 (run) ...
    const float2 *iq;      // ... or complex64 (run_iq)
    size_t stride;
    int n, n_max, C, nbb;
    double symtime;        // symbol_rate / sample_rate (a Python float)
    const float *bb;       // [nbb]
    const float *mmse;     // [129][8]
    DiscState *st;
    int *go;               // [C] 1 = this call runs the demodulator
    double2 *pc;           // [C][n_max] (phase, correction)
    float *w;              // [C][n_max] DC-tracked samples
    float *f;              // [C][n_max] low-passed samples
    float *disc;           // [C][stride] optional disc audio out (run_iq)
    uint8_t *dibits;
    size_t cap;
    int32_t *counts;
    unsigned act[MASK_WORDS];
};

__device__ __forceinline__ bool active(const DiscArgs &a, int c) { return (a.act[c >> 5] >> (c & 31)) & 1u; }

__device__ __forceinline__ double rd_lane(double v, int j) {
    long long b = __double_as_longlong(v);
    int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), j), hi = __builtin_amdgcn_readlane((int)(b >> 32), j);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ float rd_lane(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// numpy's float remainder (npy_divmod): fmod, then moved into the sign of the divisor
__device__ __forceinline__ double py_mod(double x, double y) {
    double m = fmod(x, y);
    if (m != 0.0) {
        if ((y < 0.0) != (m < 0.0)) m = __dadd_rn(m, y);
    } else {
        m = copysign(0.0, y);
    }
    return m;
}

__global__ __launch_bounds__(TILE) void k_disc_angle(DiscArgs a) {
    const int c = blockIdx.y, i = blockIdx.x * TILE + threadIdx.x;
    if (!active(a, c) || i >= a.n) return;
    const float2 *x = a.iq + (size_t)c * a.stride;
    const float2 v = x[i];
    const double p = atan2((double)v.y, (double)v.x);
    double prev;
    if (i == 0) {
        prev = a.st[c].last_phase;
    } else {
        const float2 u = x[i - 1];
        prev = atan2((double)u.y, (double)u.x);
    }
    const double dd = __dsub_rn(p, prev);
    double ddmod = __dadd_rn(py_mod(__dsub_rn(dd, -PI_D), 2.0 * PI_D), -PI_D);
    if (ddmod == -PI_D && dd > 0.0) ddmod = PI_D;
    const double corr = fabs(dd) < PI_D ? 0.0 : __dsub_rn(ddmod, dd);
    a.pc[(size_t)c * a.n_max + i] = make_double2(p, corr);
}

// IQ = true: the row is complex64 IQ (discriminator first); false: the row is float32 disc audio.
template <bool IQ>
__global__ __launch_bounds__(64) void k_disc_prep(DiscArgs a) {
    const int c = blockIdx.x, lane = threadIdx.x, n = a.n;
    if (!active(a, c)) {
        if (lane == 0) a.go[c] = 0;
        return;
    }
    // gate (system.py:658-669, p25.py:2340-2342): a non-finite sample drops the whole call, state untouched
    bool bad = false;
    float mx = 0.0f;
    if constexpr (IQ) {
        const float2 *x = a.iq + (size_t)c * a.stride;
        for (int i = lane; i < n; i += 64) {
            float2 v = x[i];
            bad |= !isfinite(v.x) || !isfinite(v.y);
        }
    } else {
        const float *x = a.audio + (size_t)c * a.stride;
        for (int i = lane; i < n; i += 64) {
            float v = x[i];
            bad |= !isfinite(v);
            mx = fmaxf(mx, fabsf(v));
        }
    }
    if (__any(bad)) {
        if (lane == 0) a.go[c] = 0;
        return;
    }
    DiscState S = a.st[c];
    float *w = a.w + (size_t)c * a.n_max;
    const float *src = a.audio + (size_t)c * a.stride;
    if constexpr (IQ) {
        // np.unwrap's cumsum of the corrections (sequential float64), up = phase + cumsum, disc = diff(up)
        const double2 *pc = a.pc + (size_t)c * a.n_max;
        float *dout = a.disc ? a.disc + (size_t)c * a.stride : nullptr;
        double csum = 0.0, up_prev = S.last_phase;
        for (int base = 0; base < n; base += 64) {
            const int cnt = min(64, n - base);
            const double2 q = lane < cnt ? pc[base + lane] : make_double2(0.0, 0.0);
            float mine = 0.0f;
            for (int j = 0; j < cnt; ++j) {
                const double p = rd_lane(q.x, j), corr = rd_lane(q.y, j);
                csum = (base + j == 0) ? corr : __dadd_rn(csum, corr);
                const double up = __dadd_rn(p, csum);
                const float d = (float)__dsub_rn(up, up_prev);
                up_prev = up;
                if (lane == j) mine = d;
            }
            if (lane < cnt) {
                w[base + lane] = mine;
                if (dout) dout[base + lane] = mine;
                mx = fmaxf(mx, fabsf(mine));
            }
        }
        S.last_phase = up_prev;
        src = w;
    }
    mx = wave_max(mx);
    // auto-gain (p25.py:1218-1227); max|x| > 0.01 is a float32 comparison with the Python float cast to float32
    if (n > 100 && mx > (float)0.01) {
        const float ng = __fdiv_rn(3.0f, mx);
        const float g9 = S.gain_f ? __fmul_rn((float)S.gain, (float)0.9) : (float)__dmul_rn(S.gain, 0.9);
        S.gain = (double)__fadd_rn(g9, __fmul_rn(ng, (float)0.1));
        S.gain_f = 1;
    }
    const float gs = (float)S.gain;
    // DC tracker (p25.py:1229-1235): dc = dc * (1 - alpha) + s * alpha, then s - dc, sequential float32
    const float ALPHA_F = (float)0.001, OMA_F = (float)(1.0 - 0.001);
    float dc = (float)S.dc;
    for (int base = 0; base < n; base += 64) {
        const int cnt = min(64, n - base);
        const float s = lane < cnt ? __fmul_rn(src[base + lane], gs) : 0.0f;
        const float pr = __fmul_rn(s, ALPHA_F);
        float mine = 0.0f;
        int j = 0;
        if (!S.dc_f && cnt > 0) {           // first sample after a reset: dc is the Python float S.dc
            dc = __fadd_rn((float)__dmul_rn(S.dc, 1.0 - 0.001), rd_lane(pr, 0));
            if (lane == 0) mine = __fsub_rn(s, dc);
            S.dc_f = 1;
            j = 1;
        }
        for (; j < cnt; ++j) {
            dc = __fadd_rn(__fmul_rn(dc, OMA_F), rd_lane(pr, j));
            const float y = __fsub_rn(rd_lane(s, j), dc);
            if (lane == j) mine = y;
        }
        if (lane < cnt) w[base + lane] = mine;
    }
    if (n > 0) S.dc = (double)dc;
    if (lane == 0) {
        a.st[c] = S;
        a.go[c] = 1;
    }
}

__global__ __launch_bounds__(TILE) void k_disc_lpf(DiscArgs a) {
    __shared__ float xs[TILE + MAX_BB - 1];
    __shared__ double hs[MAX_BB];
    const int c = blockIdx.y, t = threadIdx.x, base = blockIdx.x * TILE;
    if (!a.go[c]) return;
    const float *x = a.w + (size_t)c * a.n_max;
    float *y = a.f + (size_t)c * a.n_max;
    const int L = a.nbb, half = (L - 1) / 2, i = base + t;
    if (a.n < L) {   // p25.py:1238: no filter on a short call
        if (i < a.n) y[i] = x[i];
        return;
    }
    for (int k = t; k < L; k += TILE) hs[k] = (double)a.bb[k];
    for (int j = t; j < TILE + L - 1; j += TILE) {
        const int s = base - (L - 1 - half) + j;   // 'same': out[i] = sum_k h[k] x[i + half - k]
        xs[j] = (s >= 0 && s < a.n) ? x[s] : 0.0f;
    }
    __syncthreads();
    if (i >= a.n) return;
    double acc = 0.0;
    for (int k = 0; k < L; ++k) acc = fma(hs[k], (double)xs[t + L - 1 - k], acc);
    y[i] = (float)acc;
}

__device__ __forceinline__ float mmse_interp(const float *mm, const float *win, int oldest, int imu) {
    float r = 0.0f;   // result = 0.0 (Python float) + float32 products, one at a time (p25.py:1245-1253)
#pragma unroll
    for (int t = 0; t < NT; ++t) r = __fadd_rn(r, __fmul_rn(mm[imu * NT + t], win[(oldest + t) & 127]));
    return r;
}

__device__ __forceinline__ int mu_index(bool f32, float m32, double m64) {   // min(round(mu * 128), 128)
    int k;
    if (f32) {
        const float v = rintf(__fmul_rn(m32, (float)NSTEPS));
        k = v >= 0.0f ? (v < (float)NSTEPS ? (int)v : NSTEPS) : 0;
    } else {
        const double v = rint(__dmul_rn(m64, (double)NSTEPS));
        k = v >= 0.0 ? (v < (double)NSTEPS ? (int)v : NSTEPS) : 0;
    }
    return k;   // a NaN clock maps to 0 (unreachable: the rows are finite) -- never an out-of-table index
}

__global__ __launch_bounds__(64) void k_disc_sym(DiscArgs a) {
    __shared__ float mm[(NSTEPS + 1) * NT];
    __shared__ float win[128];
    const int c = blockIdx.x, lane = threadIdx.x, n = a.n;
    if (!a.go[c]) {
        if (lane == 0) a.counts[c] = 0;
        return;
    }
    for (int j = lane; j < (NSTEPS + 1) * NT; j += 64) mm[j] = a.mmse[j];
    DiscState S = a.st[c];
    const float *y = a.f + (size_t)c * a.n_max;
    if (lane < NT) win[(120 + lane) & 127] = S.hist[lane];   // samples -8 .. -1
    uint8_t *dib = a.dibits + (size_t)c * a.cap;
    const float ST32 = (float)a.symtime;
    const float K_SPREAD = (float)0.01, K_TIMING = (float)0.025, K_FINE = (float)0.125, K_COARSE = (float)0.00125;
    const float SPREAD_MAX = (float)2.4, SPREAD_MIN = (float)1.6;
    // typed copies of the loop variables
    double clock64 = S.clock, spread64 = S.spread, fine64 = S.fine, coarse64 = S.coarse;
    float clock32 = (float)S.clock, spread32 = (float)S.spread, fine32 = (float)S.fine, coarse32 = (float)S.coarse;
    bool clock_f = S.clock_f, spread_f = S.spread_f, fine_f = S.fine_f, coarse_f = S.coarse_f;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        __syncthreads();
        if (base + lane < n) win[(base + lane) & 127] = y[base + lane];
        __syncthreads();
        const int end = min(n, base + 64);
        for (int i = base; i < end; ++i) {
            bool fire;
            if (!clock_f) {
                clock64 = __dadd_rn(clock64, a.symtime);
                fire = clock64 > 1.0;
            } else {
                clock32 = __fadd_rn(clock32, ST32);
                fire = clock32 > 1.0f;
            }
            if (!fire) continue;
            // mu = clock / symbol_time; mu = min(mu, 1.0)
            bool mu_f;
            float mu32 = 0.0f;
            double mu64 = 0.0;
            if (!clock_f) {
                clock64 = __dsub_rn(clock64, 1.0);
                mu64 = __ddiv_rn(clock64, a.symtime);
                if (1.0 < mu64) mu64 = 1.0;
                mu_f = false;
            } else {
                clock32 = __fsub_rn(clock32, 1.0f);
                mu32 = __fdiv_rn(clock32, ST32);
                mu_f = !(1.0f < mu32);
                if (!mu_f) mu64 = 1.0;
            }
            const int imu = mu_index(mu_f, mu32, mu64);
            // mu_p1 = min(mu + 1/128, 1.0)
            bool p1_f = mu_f;
            float p1_32 = 0.0f;
            double p1_64 = 0.0;
            if (mu_f) {
                p1_32 = __fadd_rn(mu32, 1.0f / NSTEPS);
                if (1.0f < p1_32) { p1_64 = 1.0; p1_f = false; }
            } else {
                p1_64 = __dadd_rn(mu64, 1.0 / NSTEPS);
                if (1.0 < p1_64) p1_64 = 1.0;
            }
            const int imu1 = mu_index(p1_f, p1_32, p1_64);
            const int oldest = i - (NT - 1);
            float interp = mmse_interp(mm, win, oldest, imu);
            float interp_p1 = mmse_interp(mm, win, oldest, imu1);
            const float fine_v = fine_f ? fine32 : (float)fine64;
            interp = __fsub_rn(interp, fine_v);
            interp_p1 = __fsub_rn(interp_p1, fine_v);
            const float sp = spread_f ? spread32 : (float)spread64;   // spread as it meets a float32
            const float output = __fdiv_rn(__fmul_rn(2.0f, interp), sp);
            const float m15 = spread_f ? __fmul_rn(1.5f, spread32) : (float)__dmul_rn(1.5, spread64);
            const float m05 = spread_f ? __fmul_rn(0.5f, spread32) : (float)__dmul_rn(0.5, spread64);
            float err;
            if (interp < -sp) err = __fadd_rn(interp, m15);
            else if (interp < 0.0f) err = __fadd_rn(interp, m05);
            else if (interp < sp) err = __fsub_rn(interp, m05);
            else err = __fsub_rn(interp, m15);
            float ns;
            if (interp < -sp || interp >= sp) ns = __fsub_rn(sp, __fmul_rn(__fmul_rn(err, 0.5f), K_SPREAD));
            else if (interp < 0.0f) ns = __fsub_rn(sp, __fmul_rn(err, K_SPREAD));
            else ns = __fadd_rn(sp, __fmul_rn(err, K_SPREAD));
            // max(1.6, min(2.4, ns)): the Python literal wins unless ns is strictly inside
            if (ns < SPREAD_MAX) {
                if (ns > SPREAD_MIN) { spread32 = ns; spread_f = true; }
                else { spread64 = 1.6; spread_f = false; }
            } else {
                spread64 = 2.4; spread_f = false;
            }
            // timing
            const float tstep = __fmul_rn(err, K_TIMING);
            const float cv = clock_f ? clock32 : (float)clock64;
            clock32 = interp_p1 < interp ? __fadd_rn(cv, tstep) : __fsub_rn(cv, tstep);
            clock_f = true;
            // coarse += (fine - coarse) * K (float64 only while both are Python floats), then fine += err * K
            if (!fine_f && !coarse_f) {
                coarse64 = __dadd_rn(coarse64, __dmul_rn(__dsub_rn(fine64, coarse64), 0.00125));
            } else {
                const float cc = coarse_f ? coarse32 : (float)coarse64;
                coarse32 = __fadd_rn(cc, __fmul_rn(__fsub_rn(fine_v, cc), K_COARSE));
                coarse_f = true;
            }
            fine32 = __fadd_rn(fine_v, __fmul_rn(err, K_FINE));
            fine_f = true;
            int dibit;
            if (output < -2.0f) dibit = 3;
            else if (output < 0.0f) dibit = 2;
            else if (output < 2.0f) dibit = 0;
            else dibit = 1;
            if ((size_t)count < a.cap && lane == 0) dib[count] = (uint8_t)dibit;
            ++count;
        }
    }
    __syncthreads();
    if (lane == 0) {
        if (n > 0)
            for (int t = 0; t < NT; ++t) S.hist[t] = win[(n - NT + t) & 127];
        S.hist_idx = (int)((S.hist_idx + (long long)n) % NT);
        S.symbol_count += count;
        S.clock = clock_f ? (double)clock32 : clock64;
        S.spread = spread_f ? (double)spread32 : spread64;
        S.fine = fine_f ? (double)fine32 : fine64;
        S.coarse = coarse_f ? (double)coarse32 : coarse64;
        S.clock_f = clock_f; S.spread_f = spread_f; S.fine_f = fine_f; S.coarse_f = coarse_f;
        a.st[c] = S;
        a.counts[c] = count;
    }
}

DiscState fresh_state() {
    DiscState s{};
    s.spread = 2.0;
    s.gain = 1.0;
    return s;
}

}  // namespace

struct wh_disc_bank {
    int C, n_max, nbb;
    double symtime;
    DevBuf<float> d_bb, d_mmse;
    DevBuf<DiscState> d_st;
    DevBuf<int> d_go;
    DevBuf<double2> d_pc;
    DevBuf<float> d_w, d_f;
};

static int disc_alloc_work(wh_disc_bank *b, int n_max, hipStream_t st) {
    DevBuf<double2> pc;
    DevBuf<float> w, f;
    const size_t m = (size_t)b->C * (size_t)n_max;
    hipError_t e = pc.alloc(m);
    if (e == hipSuccess) e = w.alloc(m);
    if (e == hipSuccess) e = f.alloc(m);
    if (e == hipSuccess) e = sync_before_swap(st);
    if (e != hipSuccess)
        return set_err(WH_E_HIP, "wh_disc_bank: work buffers of %d x %d samples -> %s", b->C, n_max, hipGetErrorString(e));
    b->d_pc = std::move(pc); b->d_w = std::move(w); b->d_f = std::move(f);
    b->n_max = n_max;
    return WH_OK;
}

extern "C" int wh_disc_bank_create(wh_disc_bank **out, int n_channels, double sample_rate, double symbol_rate,
                                   const float *h_bb_taps, int n_bb, const float *h_mmse, size_t max_samples_per_call) {
    if (!out || !h_bb_taps || !h_mmse || n_channels < 1 || n_channels > WH_DISC_MAX_CHANNELS || !(sample_rate > 0.0) ||
        !(sample_rate < 1e9) || !(symbol_rate > 0.0) || !(symbol_rate < sample_rate) || n_bb < 1 || n_bb > MAX_BB ||
        n_bb % 2 == 0 || max_samples_per_call < 1 || max_samples_per_call > (size_t)1 << 26)
        return set_err(WH_E_ARG, "wh_disc_bank_create: bad arguments (1..%d channels, odd n_bb <= %d, "
                                 "1 <= max_samples_per_call <= 2^26)", WH_DISC_MAX_CHANNELS, MAX_BB);
    std::unique_ptr<wh_disc_bank> b(new wh_disc_bank());
    b->C = n_channels; b->nbb = n_bb; b->n_max = 0;
    b->symtime = symbol_rate / sample_rate;
    WH_HIP(b->d_bb.alloc(n_bb));
    WH_HIP(b->d_mmse.alloc((NSTEPS + 1) * NT));
    WH_HIP(hipMemcpy(b->d_bb, h_bb_taps, n_bb * sizeof(float), hipMemcpyHostToDevice));
    WH_HIP(hipMemcpy(b->d_mmse, h_mmse, (NSTEPS + 1) * NT * sizeof(float), hipMemcpyHostToDevice));
    WH_HIP(b->d_st.alloc((size_t)n_channels));
    WH_HIP(b->d_go.alloc((size_t)n_channels));
    int rc = disc_alloc_work(b.get(), (int)max_samples_per_call, nullptr);
    if (rc != WH_OK) return rc;
    std::vector<DiscState> z((size_t)n_channels, fresh_state());
    WH_HIP(hipMemcpy(b->d_st, z.data(), z.size() * sizeof(DiscState), hipMemcpyHostToDevice));
    *out = b.release();
    return WH_OK;
}

extern "C" void wh_disc_bank_destroy(wh_disc_bank *b) { delete b; }

// Only the per-call work buffers depend on the call length; the carried state does not, so a longer call than the bank
// was created for grows them and keeps every channel's state.  Synchronises the stream and the device (a steady caller
// never grows).
extern "C" int wh_disc_bank_reserve(wh_disc_bank *b, size_t max_samples_per_call, void *stream) {
    if (!b || max_samples_per_call < 1 || max_samples_per_call > (size_t)1 << 26)
        return set_err(WH_E_ARG, "wh_disc_bank_reserve: bad arguments");
    if (max_samples_per_call <= (size_t)b->n_max) return WH_OK;
    return disc_alloc_work(b, (int)max_samples_per_call, as_stream(stream));
}

// full = 0: DiscriminatorDemodulator.reset() (p25.py:1335-1345; keeps the input gain, and the recorder keeps its phase);
// full = 1: a fresh recorder assignment (a new P25Decoder, system.py:446, and _last_phase = 0.0, :389).
extern "C" int wh_disc_bank_reset(wh_disc_bank *b, int channel, int full, void *stream) {
    if (!b || channel < -1 || channel >= b->C || (full != 0 && full != 1))
        return set_err(WH_E_ARG, "wh_disc_bank_reset: bad arguments");
    hipStream_t st = as_stream(stream);
    const int c0 = channel < 0 ? 0 : channel, nc = channel < 0 ? b->C : 1;
    std::vector<DiscState> s((size_t)nc);
    WH_HIP(hipStreamSynchronize(st));
    WH_HIP(hipMemcpy(s.data(), b->d_st + c0, nc * sizeof(DiscState), hipMemcpyDeviceToHost));
    for (DiscState &x : s) {
        DiscState y = fresh_state();
        if (!full) {
            y.gain = x.gain;
            y.gain_f = x.gain_f;
            y.last_phase = x.last_phase;
        }
        x = y;
    }
    WH_HIP(hipMemcpy(b->d_st + c0, s.data(), nc * sizeof(DiscState), hipMemcpyHostToDevice));
    return WH_OK;
}

// h_out[23] = clock, spread, dc, fine, coarse, gain, last_phase, then their six float32 flags (clock, spread, dc, fine,
// coarse, gain), hist_idx, symbol_count, hist[8] in the reference's ring layout (_history).
extern "C" int wh_disc_bank_get_state(wh_disc_bank *b, int channel, double *h_out, void *stream) {
    if (!b || !h_out || channel < 0 || channel >= b->C) return set_err(WH_E_ARG, "wh_disc_bank_get_state: bad arguments");
    DiscState s;
    WH_HIP(hipStreamSynchronize(as_stream(stream)));
    WH_HIP(hipMemcpy(&s, b->d_st + channel, sizeof(s), hipMemcpyDeviceToHost));
    const double v[15] = {s.clock, s.spread, s.dc, s.fine, s.coarse, s.gain, s.last_phase,
                          (double)s.clock_f, (double)s.spread_f, (double)s.dc_f, (double)s.fine_f, (double)s.coarse_f,
                          (double)s.gain_f, (double)s.hist_idx, (double)s.symbol_count};
    for (int k = 0; k < 15; ++k) h_out[k] = v[k];
    for (int t = 0; t < NT; ++t) h_out[15 + (s.hist_idx + t) % NT] = s.hist[t];
    return WH_OK;
}

static int disc_run(wh_disc_bank *b, const char *fn, const float *d_in, bool iq, size_t n, size_t stride,
                    const uint8_t *h_active, float *d_disc, uint8_t *d_dibits, size_t cap, int32_t *d_counts,
                    void *stream) {
    if (!b || !d_counts) return set_err(WH_E_ARG, "%s: null handle/counts", fn);
    hipStream_t st = as_stream(stream);
    if (n == 0) {   // the reference raises here (disc_audio.min() of an empty array); a no-op instead
        WH_HIP(hipMemsetAsync(d_counts, 0, (size_t)b->C * sizeof(int32_t), st));
        return WH_OK;
    }
    if (!d_in || !d_dibits) return set_err(WH_E_ARG, "%s: null buffer", fn);
    if (n > (size_t)b->n_max) return set_err(WH_E_ARG, "%s: n = %zu exceeds max_samples_per_call %d (reserve first)", fn, n, b->n_max);
    if (stride < n) return set_err(WH_E_ARG, "%s: stride < n", fn);
    if (cap < n) return set_err(WH_E_ARG, "%s: cap must be >= n (at most one symbol per sample)", fn);
    DiscArgs a{};
    a.audio = iq ? nullptr : d_in;
    a.iq = iq ? reinterpret_cast<const float2 *>(d_in) : nullptr;
    a.stride = stride;
    a.n = (int)n; a.n_max = b->n_max; a.C = b->C; a.nbb = b->nbb;
    a.symtime = b->symtime;
    a.bb = b->d_bb; a.mmse = b->d_mmse;
    a.st = b->d_st; a.go = b->d_go; a.pc = b->d_pc; a.w = b->d_w; a.f = b->d_f;
    a.disc = d_disc;
    a.dibits = d_dibits; a.cap = cap; a.counts = d_counts;
    for (int k = 0; k < b->C; ++k)
        if (!h_active || h_active[k]) a.act[k >> 5] |= 1u << (k & 31);
    const dim3 tiles((unsigned)((n + TILE - 1) / TILE), (unsigned)b->C);
    if (iq) {
        hipLaunchKernelGGL(k_disc_angle, tiles, dim3(TILE), 0, st, a);
        WH_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_disc_prep<true>, dim3(b->C), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_disc_prep<false>, dim3(b->C), dim3(64), 0, st, a);
    }
    WH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_disc_lpf, tiles, dim3(TILE), 0, st, a);
    WH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_disc_sym, dim3(b->C), dim3(64), 0, st, a);
    WH_LAUNCH_CHECK();
    return WH_OK;
}

extern "C" int wh_disc_bank_run(wh_disc_bank *b, const float *d_audio, size_t n, size_t stride, const uint8_t *h_active,
                                uint8_t *d_dibits, size_t cap, int32_t *d_counts, void *stream) {
    return disc_run(b, "wh_disc_bank_run", d_audio, false, n, stride, h_active, nullptr, d_dibits, cap, d_counts, stream);
}

extern "C" int wh_disc_bank_run_iq(wh_disc_bank *b, const float *d_iq, size_t n, size_t stride, const uint8_t *h_active,
                                   float *d_disc, uint8_t *d_dibits, size_t cap, int32_t *d_counts, void *stream) {
    return disc_run(b, "wh_disc_bank_run_iq", d_iq, true, n, stride, h_active, d_disc, d_dibits, cap, d_counts, stream);
}
