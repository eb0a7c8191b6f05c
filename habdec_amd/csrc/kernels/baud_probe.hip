// Baud-rate probe (hd_baud_probe_*, include/habdec_amd.h has the definition; host/baud_probe.hpp restates it sample by sample).  Not in the reference.
//
// k_baud_probe: one workgroup per stream, candidate k on thread k (sixteen waves; the candidates ascend in frequency, so a wave's 64 listen to one scale
// or to two neighbouring ones).  Every wave walks the push in steps of the 64 samples of one history word: the lanes compare, __ballot makes the sign
// word, and for each scale the wave needs the window counts come from prefix popcounts over the 512-bit history plus the word in the making -- the
// words and their cumulative counts are wave-uniform and lie in the wave's own corner of LDS, a lane masks and counts the two words its window ends
// in.  A second ballot turns the majority bits into a word, one XOR into the step's edge mask: wave-uniform, so the loop over its edges is a scalar
// loop in which a lane adds to its own candidate.  Accumulators are loaded once and stored once per push.  Integer arithmetic from the comparison on,
// no atomics: the same pushes give the same bits, whatever the launch looks like.
//
// One arithmetic, like survey.hip: not compiled per mode.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "wave_util.h"

namespace hd {

namespace {

__device__ __forceinline__ uint64_t low_mask(uint32_t x) { return x >= 64u ? ~0ull : (1ull << x) - 1ull; }      // bits [0, x)
// the lanes of a wave exchange data through its own LDS rows: LDS operations of one wave execute in order, the compiler must keep them in order too
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Acc {
    uint64_t P, Q;
    uint32_t NB, n, cur;
    int32_t re, im;
};

__device__ __forceinline__ void edge(Acc& c, const uint64_t i, const uint32_t F, const int32_t* C)
{
    const uint64_t p = i * (uint64_t)F;
    const uint32_t idx = (uint32_t)(p >> 22) & 1023u, block = (uint32_t)(p >> 38);
    if (block != c.cur) {
        if (c.n >= 8u && c.n <= 4096u) {
            c.P += (uint64_t)((int64_t)c.re * c.re) + (uint64_t)((int64_t)c.im * c.im);
            c.Q += (uint64_t)c.n * c.n;
            c.NB += 1u;
        }
        c.re = c.im = 0;
        c.n = 0;
        c.cur = block;
    }
    c.n += 1u;
    if (c.n <= 4096u) { c.re += C[idx]; c.im += C[(idx + 768u) & 1023u]; }
}

}  // namespace

__global__ __launch_bounds__(1024) void k_baud_probe(const ProbeSrc* __restrict__ src, hd_baud_probe_stream_state* __restrict__ hdr,
                                                      unsigned long long* __restrict__ acc64, uint32_t* __restrict__ acc32,
                                                      const uint32_t* __restrict__ Ftab, const uint32_t* __restrict__ scale_tab,
                                                      const int32_t* __restrict__ ctab)
{
    __shared__ int32_t C[1024];
    // Per wave: the history as a ring of sixteen 64-bit words -- word c (samples 64 c .. 64 c + 63) in slot c & 15, so that the word in the making, the
    // seven in front of it and the one it replaces in the stream's eight-word state (word c - 8) all have a slot -- and cw[j] = set bits in words
    // c - 8 .. c - 9 + j.
    __shared__ uint64_t hw_all[16][16];
    __shared__ uint32_t cw_all[16][16];
    const uint32_t s = blockIdx.x, t = threadIdx.x, l = t & 63u, wave = uni32(t >> 6);
    const ProbeSrc d = src[s];
    const uint32_t n = uni32(d.n);
    if (!n) return;                                                  // (the whole workgroup: nothing of this stream changes)
    hd_baud_probe_stream_state* H = hdr + s;
    uint64_t* hw = hw_all[wave];
    uint32_t* cw = cw_all[wave];
    C[t] = ctab[t];
    const uint64_t i0 = uni64(H->samples);
    uint32_t first = 0;
    if (d.ring_mask) first = (d.sym->base + d.sym->held - n) & d.ring_mask;      // the ring's append position is base + held: the call's output ends there

    // ---- this thread's candidate
    unsigned long long* a64 = acc64 + (size_t)s * 2u * HD_PROBE_CANDIDATES;
    uint32_t* a32 = acc32 + (size_t)s * 5u * HD_PROBE_CANDIDATES;
    Acc c;
    c.P = a64[t]; c.Q = a64[HD_PROBE_CANDIDATES + t];
    c.NB = a32[t]; c.re = (int32_t)a32[HD_PROBE_CANDIDATES + t]; c.im = (int32_t)a32[2 * HD_PROBE_CANDIDATES + t];
    c.n = a32[3 * HD_PROBE_CANDIDATES + t]; c.cur = a32[4 * HD_PROBE_CANDIDATES + t];
    const uint32_t F = Ftab[t], my_scale = scale_tab[t];
    // the scales this wave computes: those of its candidates (a run: the table descends), and scale `wave` for the stream's header
    const uint32_t sc_hi = uni32(my_scale), sc_lo = (uint32_t)__builtin_amdgcn_readlane((int)my_scale, 63);
    uint32_t need = (2u << sc_hi) - (1u << sc_lo);
    if (wave < HD_PROBE_SCALES) need |= 1u << wave;

    // ---- the stream's state: words c0 - 8 .. c0 - 1 of the history (the first of them shares its place in the state with word c0 itself)
    const uint32_t c0 = (uint32_t)(i0 >> 6);
    if (l < 8u) hw[(c0 - 8u + l) & 15u] = H->history[(c0 + l) & 7u];
    const uint64_t seed = uni64(H->history[c0 & 7u]) & low_mask((uint32_t)i0 & 63u);      // the samples of word c0 that earlier pushes brought
    uint32_t m_prev = 0, hdr_edges = 0;       // m_W[i-1] of scale k in bit k; the edges of scale `wave`, which this wave counts for the header
    for (uint32_t k = 0; k < HD_PROBE_SCALES; ++k) m_prev |= (uni32(H->majority[k]) & 1u) << k;
    __syncthreads();                                                 // the table is in LDS, and every wave has read the header that some will write

    const uint32_t n_steps = (((uint32_t)i0 & 63u) + n + 63u) >> 6;
    const uint64_t end = i0 + n;
    uint32_t e_l = 64;
    for (uint32_t st = 0; st < n_steps; ++st) {
        const uint32_t cword = c0 + st;
        const uint64_t word_base = ((i0 >> 6) + st) << 6;
        const uint32_t s_l = st ? 0u : (uint32_t)i0 & 63u;
        e_l = end - word_base >= 64u ? 64u : (uint32_t)(end - word_base);
        const bool valid = l >= s_l && l < e_l;
        float v = 0.0f;
        if (valid) {
            const uint32_t j = (uint32_t)(word_base + l - i0);      // < n
            v = d.ring_mask ? d.p[(first + j) & d.ring_mask] : d.p[j];
        }
        const uint64_t cur = (st ? 0ull : seed) | __ballot(valid && v > 0.0f);      // (NaN compares false; bits from the step's last lane on are zero)
        if (l == 0) hw[cword & 15u] = cur;
        wave_lds_sync();
        if (l < 10u) {
            uint32_t sum = 0;
            for (uint32_t k = 0; k < l; ++k) sum += (uint32_t)__popcll(hw[(cword - 8u + k) & 15u]);
            cw[l] = sum;
        }
        wave_lds_sync();
        // the window of lane l ends at position 512 + l of the nine words' 576 and starts behind position 512 + l - W
        const uint32_t top = cw[8] + (uint32_t)__popcll(cur & low_mask(l + 1u));
        for (uint32_t rest = need; rest; rest &= rest - 1u) {
            const uint32_t sc = (uint32_t)__builtin_ctz(rest), W = (2u << sc) - 1u;
            const uint32_t u = 512u - W + l, j = u >> 6;
            const uint32_t count = top - (cw[j] + (uint32_t)__popcll(hw[(cword - 8u + j) & 15u] & low_mask((u & 63u) + 1u)));
            const uint64_t M = __ballot(count > (W - 1u) / 2u);
            const uint64_t prev = ((M & ~low_mask(s_l)) << 1) | ((uint64_t)((m_prev >> sc) & 1u) << s_l);
            const uint64_t old_enough = word_base >= W ? ~0ull : ~low_mask(W - (uint32_t)word_base);       // an edge needs i >= W
            m_prev = (m_prev & ~(1u << sc)) | (((uint32_t)(M >> (e_l - 1u)) & 1u) << sc);
            uint64_t E = (M ^ prev) & low_mask(e_l) & ~low_mask(s_l) & old_enough;
            if (wave == sc) hdr_edges += (uint32_t)__popcll(E);
            if (sc < sc_lo || sc > sc_hi) continue;                  // (computed for the header only)
            const bool mine = my_scale == sc;
            while (E) {
                const uint32_t b = (uint32_t)__builtin_ctzll(E);
                E &= E - 1ull;
                if (mine) edge(c, word_base + b, F, C);
            }
        }
        wave_lds_sync();                                             // (the next step's stores come behind this step's loads)
    }

    __syncthreads();                                                 // (belt and braces: no wave writes the header while another could still read it)
    a64[t] = c.P; a64[HD_PROBE_CANDIDATES + t] = c.Q;
    a32[t] = c.NB; a32[HD_PROBE_CANDIDATES + t] = (uint32_t)c.re; a32[2 * HD_PROBE_CANDIDATES + t] = (uint32_t)c.im;
    a32[3 * HD_PROBE_CANDIDATES + t] = c.n; a32[4 * HD_PROBE_CANDIDATES + t] = c.cur;
    if (wave < HD_PROBE_SCALES) {
        if (l == 0) {
            H->majority[wave] = (m_prev >> wave) & 1u;
            H->edges[wave] += hdr_edges;
        }
    } else if (wave == HD_PROBE_SCALES) {
        // the last word's place in the state keeps the bits of the word it replaces behind the last sample; the seven words in front of it go whole
        const uint32_t c_last = c0 + n_steps - 1u;
        if (l == 0) {
            H->history[c_last & 7u] = (hw[c_last & 15u] & low_mask(e_l)) | (hw[(c_last - 8u) & 15u] & ~low_mask(e_l));
            H->samples = end;
        } else if (l < 8u) H->history[(c_last + l) & 7u] = hw[(c_last - 8u + l) & 15u];
    }
}

void launch_baud_probe(hipStream_t st, uint32_t n_streams, const ProbeSrc* src, hd_baud_probe_stream_state* hdr, unsigned long long* acc64, uint32_t* acc32,
                       const uint32_t* F, const uint32_t* scale, const int32_t* ctab)
{
    hipLaunchKernelGGL(k_baud_probe, dim3(n_streams), dim3(1024), 0, st, src, hdr, acc64, acc32, F, scale, ctab);
}

}  // namespace hd
