// mlp_k2_f16x1_to.hip - C-ABI precision 5, the sampler's SDF queries: K2 with ONE MFMA per product in TILE-OUTER order, 32 points per wave.
//
// mlp_chain_f16x1.hip walks a layer k-step outer / output tile inner: every weight fragment read from LDS feeds ONE MFMA (16 points per wave) and two full
// fp32 accumulator sets (128 VGPRs) stay live.  Here the output tile is the outer loop: a PAIR of output tiles (2p, 2p + 1) walks the layer's k-steps in
// ascending order and is final after the last one, so what stays live across a layer is the packed fp16 input units (4 VGPRs per unit per 16 points)
// and two pairs of accumulators.  That leaves room for TWO point groups per wave: every fragment read feeds two MFMAs, and per point the fragment reads,
// the counted waits, the LDS-DMA pieces, the L2 -> LDS bytes and the chunk barriers are halved.  Arithmetic per accumulator element is unchanged - bias,
// then k-steps 0, 1, ... through the same instructions (hh, hl, lh on the encoding k-steps), the same epilogue slices, the same fmaf chain of the last
// row - so the result is bit-identical to f16x1::k_sdf_only_bf16, which stays in the library as the reference (NERFART_K2_F16X1=ref).
//
//   points     m = tile * 256 + wave * 32 + grp * 16 + j
//   blob       the precision-4/5 surface blob as it is: item (k-step u, tile T) of a layer at layer base + (16 u + T) * 2 KiB, hi fragment in the first KiB
//   LDS chunk  hidden layers: 4 tiles x 8 k-steps, item (u, t) at (4 u + t) * 2 KiB: wave w copies k-step w (4 hi pieces); 4 chunks per layer
//              skip layer:    the same for k-steps 0..7 (k-step 7 = encoding unit 0: wave 7 copies its lo pieces too); k-step 8 (encoding unit 1) goes
//                             into the lo holes of k-steps 0 (its hi fragments, wave 0) and 1 (its lo fragments, wave 1)
//              layer 0:       blob chunk 0 as it is (2 k-steps x 16 tiles, hi + lo)
//   a pair     NI = 2 x k-steps items (k-step, tile of the pair); item = wait + MFMA(s) of both point groups, then the fillers: the fragment read two
//              items ahead, LDS-DMA pieces of the next chunk, a slice of the PREVIOUS pair's epilogue (items 1..12: both groups per slice), and at item
//              NI - 4 the counted asm reads of the next pair's bias (consumed behind item NI - 1's wait).
#define NERFART_F16X2 1
#define NERFART_F16X1 1
#define NERFART_K2_ONLY 1
#define b16 f16x1
#include "mlp_bf16_core.h"
#include <cstdlib>

namespace nerfart {
namespace f16x1 {

struct ToState {
    u32x4 cur[2][8], nxt[2][8];      // [point group][unit]: this layer's input units / the next layer's (hi parts)
    f32x4 acc[2][2][2];              // [pair parity][tile of the pair][point group]
    Unit enc[2][2];                  // [point group][encoding unit], hi + lo
    f32x4 bt[2], rw[2];              // the next pair's bias / (layer 7) this pair's slice of the sdf row
    Work2 w;
    float dot[2];
    u32x4 rh[3], rl[3];              // fragment ring
    unsigned addr, baddr;            // this lane's LDS byte address of the chunk's item 0 / of the layer's bias
};

// KIND 0: 8 hidden k-steps; 1: the skip layer (7 hidden + 2 encoding); 2: layer 0 (2 encoding)
template <int KIND, bool TAIL>
struct ToCfg {
    static constexpr int NKS = KIND == 0 ? 8 : (KIND == 1 ? 9 : 2), NH = KIND == 0 ? 8 : (KIND == 1 ? 7 : 0);
    static constexpr int NI = 2 * NKS, PPC = KIND == 2 ? 8 : 2, N = NI * PPC;
    static constexpr bool full(int ci) { return ci >= 0 && ci < N && ((ci % NI) >> 1) >= NH; }
    static constexpr int nfr(int ci) { return (ci >= 0 && ci < N) ? (full(ci) ? 2 : 1) : 0; }
    // counted asm reads issued behind the fragment read of chunk item ci; P0 = layer pair of the chunk's pair 0
    static constexpr int auxn(int P) { return TAIL ? (P == 7 ? 2 : 4) : 2; }
    static constexpr int naux(int ci, int P0) { return (ci >= 0 && ci < N && (ci % NI) == NI - 4) ? auxn(P0 + ci / NI) : 0; }
    static constexpr int hi_off(int ci) {
        const int pl = ci / NI, u = (ci % NI) >> 1, t = ci & 1;
        if (KIND == 2) return (16 * u + 2 * pl + t) * 2048;
        if (u < 8) return (4 * u + 2 * pl + t) * 2048;
        return (2 * pl + t) * 2048 + 1024;
    }
    static constexpr int lo_off(int ci) {
        const int pl = ci / NI, u = (ci % NI) >> 1, t = ci & 1;
        if (KIND == 1 && u == 8) return (4 + 2 * pl + t) * 2048 + 1024;
        return hi_off(ci) + 1024;
    }
};

template <int OFFH, int OFFL>
__device__ __forceinline__ void to_read_2(u32x4& fh, u32x4& fl, unsigned addr) {
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4" : "=&v"(fh), "=&v"(fl) : "v"(addr), "i"(OFFH), "i"(OFFL));
}
template <int OFF>
__device__ __forceinline__ void to_read_f(f32x4& v, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v) : "v"(addr), "i"(OFF));
}

// The item's wait for its fragment(s) and the MFMAs of BOTH point groups as one statement (see wait_mfma3): the two accumulator chains alternate, each
// keeps its own order (hh, hl, lh on the encoding k-steps).  PAD: a VALU instruction wrote an operand just before (the first item of a pair).
template <int CNT, bool PAD, bool FULL>
__device__ __forceinline__ void to_wait_mfma(const u32x4 ah, const u32x4 al, const u32x4 b0h, const u32x4 b0l, const u32x4 b1h, const u32x4 b1l,
                                             f32x4& a0, f32x4& a1) {
    if constexpr (FULL) {
        if constexpr (PAD) {
            asm volatile("s_waitcnt lgkmcnt(%8)\n\t"
                         "s_nop 1\n\t"
                         "v_mfma_f32_16x16x32_f16 %0, %2, %4, %0\n\t"
                         "v_mfma_f32_16x16x32_f16 %1, %2, %6, %1\n\t"
                         "v_mfma_f32_16x16x32_f16 %0, %2, %5, %0\n\t"
                         "v_mfma_f32_16x16x32_f16 %1, %2, %7, %1\n\t"
                         "v_mfma_f32_16x16x32_f16 %0, %3, %4, %0\n\t"
                         "v_mfma_f32_16x16x32_f16 %1, %3, %6, %1"
                         : "+v"(a0), "+v"(a1) : "v"(ah), "v"(al), "v"(b0h), "v"(b0l), "v"(b1h), "v"(b1l), "i"(CNT));
        } else {
            asm volatile("s_waitcnt lgkmcnt(%8)\n\t"
                         "v_mfma_f32_16x16x32_f16 %0, %2, %4, %0\n\t"
                         "v_mfma_f32_16x16x32_f16 %1, %2, %6, %1\n\t"
                         "v_mfma_f32_16x16x32_f16 %0, %2, %5, %0\n\t"
                         "v_mfma_f32_16x16x32_f16 %1, %2, %7, %1\n\t"
                         "v_mfma_f32_16x16x32_f16 %0, %3, %4, %0\n\t"
                         "v_mfma_f32_16x16x32_f16 %1, %3, %6, %1"
                         : "+v"(a0), "+v"(a1) : "v"(ah), "v"(al), "v"(b0h), "v"(b0l), "v"(b1h), "v"(b1l), "i"(CNT));
        }
    } else if constexpr (PAD) {
        asm volatile("s_waitcnt lgkmcnt(%5)\n\t"
                     "s_nop 1\n\t"
                     "v_mfma_f32_16x16x32_f16 %0, %2, %3, %0\n\t"
                     "v_mfma_f32_16x16x32_f16 %1, %2, %4, %1"
                     : "+v"(a0), "+v"(a1) : "v"(ah), "v"(b0h), "v"(b1h), "i"(CNT));
    } else {
        asm volatile("s_waitcnt lgkmcnt(%5)\n\t"
                     "v_mfma_f32_16x16x32_f16 %0, %2, %3, %0\n\t"
                     "v_mfma_f32_16x16x32_f16 %1, %2, %4, %1"
                     : "+v"(a0), "+v"(a1) : "v"(ah), "v"(b0h), "v"(b1h), "i"(CNT));
    }
}

// The chunk barrier, and where the pieces issued during the chunk that starts here go.  NXT, the chunk to stream: 0 hidden, 1 skip layer, 2 layer 0,
// 3 hidden or skip (next_skip).  `base` = float offset of that chunk's layer in the blob, q = its chunk index within the layer.  s carries the even
// (hi) pieces, sx the odd ones (stream_piece, under sx.lo_exec).
template <int NXT>
__device__ __forceinline__ unsigned to_acquire(Stream& s, Stream& sx, int base, int q, bool next_skip) {
    wait_glds();          // my pieces of the current chunk have landed
    __syncthreads();      // everyone's pieces landed; everyone is done reading the other buffer
    const unsigned cur = lds_addr(s.lds + s.pb * CHUNK_FLOATS), dst = lds_addr(s.lds + (s.pb ^ 1) * CHUNK_FLOATS);
    const int w = wave_id();
    s.iss_dst = dst + w * 8192;
    if constexpr (NXT == 2) {
        s.iss_src = s.blob + base + w * 2048;
        sx.iss_src = s.iss_src; sx.iss_dst = s.iss_dst; sx.lo_exec = ~0ull;
    } else {
        s.iss_src = s.blob + base + (w * 16 + 4 * q) * 512;
        if constexpr (NXT != 0) {
            // wave 7: the lo fragments of its own k-step 7.  Waves 0 / 1: k-step 8's hi / lo fragments into the holes of k-steps 0 / 1 - through the ODD pieces,
            // whose offsets are 1 KiB + 2 KiB * tile: the hi fragments' source and destination start 1 KiB lower
            const float* s8 = s.blob + base + (8 * 16 + 4 * q) * 512;
            sx.iss_src = (w == 7) ? s.iss_src : ((w == 0) ? s8 - 256 : s8);
            sx.iss_dst = (w == 7) ? s.iss_dst : ((w == 0) ? dst : dst + 8192);
            const bool on = (NXT == 1 || next_skip) && (w == 7 || w < 2);
            sx.lo_exec = __builtin_amdgcn_readfirstlane((int)on) != 0 ? ~0ull : 0ull;
        }
    }
    s.pb ^= 1;
    return cur;
}

template <int KIND, bool TAIL, int NXT, int PL, int P, int I>
struct ToItems {
    using C = ToCfg<KIND, TAIL>;
    static __device__ __forceinline__ void run(ToState& st, const Stream& s, const Stream& sx) {
        if constexpr (I < C::NI) {
            constexpr int ci = PL * C::NI + I, u = I >> 1, t = I & 1, pp = P & 1, S = ci % 3, S2 = (ci + 2) % 3, P0 = P - PL;
            constexpr bool FULL = C::full(ci);
            constexpr int PENDING = C::nfr(ci + 1) + C::naux(ci - 2, P0) + C::naux(ci - 1, P0);
            if constexpr (KIND == 2 || (KIND == 1 && u >= 7)) {
                constexpr int q = KIND == 2 ? u : u - 7;
                to_wait_mfma<PENDING, I == 0, true>(st.rh[S], st.rl[S], st.enc[0][q].h, st.enc[0][q].l, st.enc[1][q].h, st.enc[1][q].l,
                                                    st.acc[pp][t][0], st.acc[pp][t][1]);
            } else {
                to_wait_mfma<PENDING, I == 0, false>(st.rh[S], st.rh[S], st.cur[0][u], st.cur[0][u], st.cur[1][u], st.cur[1][u],
                                                     st.acc[pp][t][0], st.acc[pp][t][1]);
            }
            static_assert(FULL == (KIND == 2 || (KIND == 1 && u >= 7)), "three-term k-steps");
            if constexpr (ci + 2 < C::N) {
                if constexpr (C::full(ci + 2)) to_read_2<C::hi_off(ci + 2), C::lo_off(ci + 2)>(st.rh[S2], st.rl[S2], st.addr);
                else lds_read_hi<C::hi_off(ci + 2)>(st.rh[S2], st.addr);
            }
            constexpr bool BIAS = !(TAIL && P == 7);
            if constexpr (I == C::NI - 4) {
                // bias of the next pair (tiles 2 pn, 2 pn + 1; pair 0 of the next layer behind pair 7), layer 7: this pair's slice of the sdf row
                constexpr int pn = (P + 1) & 7, boff = (P == 7 ? 1024 : 0) + 2 * pn * 64;
                if constexpr (BIAS) { to_read_f<boff>(st.bt[0], st.baddr); to_read_f<boff + 64>(st.bt[1], st.baddr); }
                if constexpr (TAIL) { to_read_f<1024 + 2 * P * 64>(st.rw[0], st.baddr); to_read_f<1024 + 2 * P * 64 + 64>(st.rw[1], st.baddr); }
            }
            // LDS-DMA pieces of the next chunk: in the items that host no epilogue slice
            if constexpr (KIND == 2) {
                if constexpr (P == 0) stream_piece<2 * I>(s);
            } else {
                constexpr bool ODD = NXT != 0;
                if constexpr (I == 0) stream_piece<4 * PL>(s);
                if constexpr (I == 13) { stream_piece<4 * PL + 2>(s); if constexpr (ODD) stream_piece<4 * PL + 1>(sx); }
                if constexpr (I == 15) { if constexpr (ODD) stream_piece<4 * PL + 3>(sx); }
            }
            // the previous pair's epilogue: HOST 1 softplus slices -> unit P - 1 of the next layer (pair 0: unit 7 of THIS layer's input, the previous
            // layer's last pair), HOST 2 (layer 7) its share of the sdf row's dot product
            constexpr int HOST = TAIL ? (P == 0 ? 1 : 2) : ((KIND != 0 && P == 0) ? 0 : 1);
            if constexpr (HOST == 1 && KIND == 2) {
                constexpr int pr = I, tt = pr >> 1, r0 = 2 * (pr & 1);
                unsigned h0 = 0, l0 = 0, h1 = 0, l1 = 0, dout = 0;
                epi_phase<0, 0>(st.acc[pp ^ 1][tt][0][r0], st.acc[pp ^ 1][tt][0][r0 + 1], st.w, h0, l0, 0.f, true, 0u, dout);
                epi_phase<0, 0>(st.acc[pp ^ 1][tt][1][r0], st.acc[pp ^ 1][tt][1][r0 + 1], st.w.b, h1, l1, 0.f, true, 0u, dout);
                epi_phase<0, 1>(st.acc[pp ^ 1][tt][0][r0], st.acc[pp ^ 1][tt][0][r0 + 1], st.w, h0, l0, 0.f, true, 0u, dout);
                epi_phase<0, 1>(st.acc[pp ^ 1][tt][1][r0], st.acc[pp ^ 1][tt][1][r0 + 1], st.w.b, h1, l1, 0.f, true, 0u, dout);
                epi_phase<0, 2>(0.f, 0.f, st.w, h0, l0, 0.f, true, 0u, dout);
                epi_phase<0, 2>(0.f, 0.f, st.w.b, h1, l1, 0.f, true, 0u, dout);
                st.nxt[0][P - 1][pr] = h0;
                st.nxt[1][P - 1][pr] = h1;
            }
            if constexpr (HOST == 1 && KIND != 2 && I >= 1 && I <= 12) {
                constexpr int pr = (I - 1) / 3, ph = (I - 1) % 3, tt = pr >> 1, r0 = 2 * (pr & 1);
                unsigned h0 = 0, l0 = 0, h1 = 0, l1 = 0, dout = 0;
                epi_phase<0, ph>(st.acc[pp ^ 1][tt][0][r0], st.acc[pp ^ 1][tt][0][r0 + 1], st.w, h0, l0, 0.f, true, 0u, dout);
                epi_phase<0, ph>(st.acc[pp ^ 1][tt][1][r0], st.acc[pp ^ 1][tt][1][r0 + 1], st.w.b, h1, l1, 0.f, true, 0u, dout);
                if constexpr (ph == 2) {
                    if constexpr (P == 0) { st.cur[0][7][pr] = h0; st.cur[1][7][pr] = h1; }
                    else { st.nxt[0][P - 1][pr] = h0; st.nxt[1][P - 1][pr] = h1; }
                }
            }
            if constexpr (HOST == 2 && I >= 1 && I <= 8) {
                constexpr int tt = (I - 1) >> 2, r = (I - 1) & 3;
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    const float a = st.acc[pp ^ 1][tt][gp][r];
                    const float y = fmaxf(a, 0.f) + __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-fabsf(a)));
                    st.dot[gp] = fmaf(y, st.rw[tt][r], st.dot[gp]);
                }
            }
            if constexpr (I == C::NI - 1) {
                // item NI - 1's wait covered the asm reads of item NI - 4; the other accumulator pair is free: the next pair starts at its bias
                if constexpr (BIAS) {
                    asm volatile("" : "+v"(st.bt[0]), "+v"(st.bt[1]));
                    st.acc[pp ^ 1][0][0] = st.bt[0]; st.acc[pp ^ 1][0][1] = st.bt[0];
                    st.acc[pp ^ 1][1][0] = st.bt[1]; st.acc[pp ^ 1][1][1] = st.bt[1];
                }
                if constexpr (TAIL) asm volatile("" : "+v"(st.rw[0]), "+v"(st.rw[1]));
            }
            __builtin_amdgcn_sched_barrier(0);
            ToItems<KIND, TAIL, NXT, PL, P, I + 1>::run(st, s, sx);
        }
    }
};

// One chunk: Q = chunk of the layer.  `base` / `q` / next_skip describe the chunk streamed meanwhile (to_acquire).
template <int KIND, bool TAIL, int NXT, int Q>
__device__ __forceinline__ void to_chunk(ToState& st, Stream& s, Stream& sx, int base, int q, bool next_skip) {
    using C = ToCfg<KIND, TAIL>;
    st.addr = to_acquire<NXT>(s, sx, base, q, next_skip) + lane_id() * 16;
    // everything the compiler itself has in flight on the LDS queue must be drained first: the counted waits assume only the ring's reads
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (C::full(0)) {
        to_read_2<C::hi_off(0), C::lo_off(0)>(st.rh[0], st.rl[0], st.addr);
        to_read_2<C::hi_off(1), C::lo_off(1)>(st.rh[1], st.rl[1], st.addr);
    } else {
        lds_read_hi<C::hi_off(0)>(st.rh[0], st.addr);
        lds_read_hi<C::hi_off(1)>(st.rh[1], st.addr);
    }
    if constexpr (KIND == 2) {
        ToItems<2, false, NXT, 0, 0, 0>::run(st, s, sx); ToItems<2, false, NXT, 1, 1, 0>::run(st, s, sx);
        ToItems<2, false, NXT, 2, 2, 0>::run(st, s, sx); ToItems<2, false, NXT, 3, 3, 0>::run(st, s, sx);
        ToItems<2, false, NXT, 4, 4, 0>::run(st, s, sx); ToItems<2, false, NXT, 5, 5, 0>::run(st, s, sx);
        ToItems<2, false, NXT, 6, 6, 0>::run(st, s, sx); ToItems<2, false, NXT, 7, 7, 0>::run(st, s, sx);
    } else {
        ToItems<KIND, TAIL, NXT, 0, 2 * Q, 0>::run(st, s, sx);
        ToItems<KIND, TAIL, NXT, 1, 2 * Q + 1, 0>::run(st, s, sx);
    }
}

// first blob chunk of surface layer l (pack_blob.hip::chunk_desc, program 3)
__device__ __forceinline__ int to_first_chunk(int l) { return l == 0 ? 0 : (l <= 4 ? 4 * l - 3 : 4 * l - 2); }

__global__ void __launch_bounds__(WG_THREADS, 2)
k_sdf_only_to(const float* __restrict__ blob, PointSrc src, float R_bg, float* __restrict__ sdf_out, int out_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int* hdr = reinterpret_cast<const int*>(blob);
    float* aux = smem + 2 * CHUNK_FLOATS;
    const int lane = lane_id(), g = lane >> 4, j = lane & 15, wv = wave_id();
    load_aux(aux, blob, hdr, SURF_AUX_FLOATS);
    const unsigned ntiles = (src.M + 255u) / 256u;
    if (blockIdx.x >= ntiles) return;
    Stream s = make_stream(blob, aux, smem, hdr[2]);
    stream_start(s);                   // blob chunk 0 = layer 0 in a burst into buffer 0
    Stream sx = s;
    const int base0 = __builtin_amdgcn_readfirstlane(s.tab[0]);
    const unsigned bl = lds_addr(aux) + g * 16;
    ToState st;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        Pt pt[2];
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            pt[gp] = fetch_point(src, tile * 256u + wv * 32 + gp * 16 + j, false);
            encode_units(pt[gp].x, pt[gp].y, pt[gp].z, g, -1, st.enc[gp]);
        }
        st.dot[0] = 0.f; st.dot[1] = 0.f;
        st.w = {};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(aux + 16 * t + 4 * g);
            st.acc[0][t][0] = b; st.acc[0][t][1] = b;
        }
        st.baddr = bl;
        to_chunk<2, false, 0, 0>(st, s, sx, __builtin_amdgcn_readfirstlane(s.tab[1]), 0, false);
#pragma unroll
        for (int u = 0; u < 7; ++u) { st.cur[0][u] = st.nxt[0][u]; st.cur[1][u] = st.nxt[1][u]; }
#pragma nounroll
        for (int L = 1; L < 7; ++L) {
            const int bL = __builtin_amdgcn_readfirstlane(s.tab[to_first_chunk(L)]), bN = __builtin_amdgcn_readfirstlane(s.tab[to_first_chunk(L + 1)]);
            st.baddr = bl + L * 1024;
            if (L == 4) {
                to_chunk<1, false, 1, 0>(st, s, sx, bL, 1, false);
                to_chunk<1, false, 1, 1>(st, s, sx, bL, 2, false);
                to_chunk<1, false, 1, 2>(st, s, sx, bL, 3, false);
                to_chunk<1, false, 0, 3>(st, s, sx, bN, 0, false);
            } else {
                to_chunk<0, false, 0, 0>(st, s, sx, bL, 1, false);
                to_chunk<0, false, 0, 1>(st, s, sx, bL, 2, false);
                to_chunk<0, false, 0, 2>(st, s, sx, bL, 3, false);
                to_chunk<0, false, 3, 3>(st, s, sx, bN, 0, L == 3);
            }
#pragma unroll
            for (int u = 0; u < 7; ++u) { st.cur[0][u] = st.nxt[0][u]; st.cur[1][u] = st.nxt[1][u]; }
        }
        {
            const int b7 = __builtin_amdgcn_readfirstlane(s.tab[to_first_chunk(7)]);
            st.baddr = bl + 7 * 1024;
            to_chunk<0, true, 0, 0>(st, s, sx, b7, 1, false);
            to_chunk<0, true, 0, 1>(st, s, sx, b7, 2, false);
            to_chunk<0, true, 0, 2>(st, s, sx, b7, 3, false);
            to_chunk<0, true, 2, 3>(st, s, sx, base0, 0, false);      // the next tile's layer 0 (streamed, never read, behind the last tile)
        }
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");               // last MFMA result -> first VALU reader
        // pair 7 of layer 7 (tiles 14, 15): nobody hosts it
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    const float a = st.acc[1][tt][gp][r];
                    const float y = fmaxf(a, 0.f) + __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-fabsf(a)));
                    st.dot[gp] = fmaf(y, st.rw[tt][r], st.dot[gp]);
                }
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            const unsigned m = tile * 256u + wv * 32 + gp * 16 + j;
            float sdf = sum_over_groups(st.dot[gp]) + aux[SURF_AUX_B8];
            // |x|^2 as the reference kernel's ISA contracts it (x x, then fma y y, then fma z z): spelled out, so that the bits do not hang on which of the
            // two products hipcc chooses to fuse here
            if (R_bg > 0.f) sdf = fminf(sdf, R_bg - sqrtf(fmaf(pt[gp].z, pt[gp].z, fmaf(pt[gp].y, pt[gp].y, pt[gp].x * pt[gp].x))));
            if (g == 0 && m < src.M) {
                if (src.pts) sdf_out[m] = sdf;
                else {
                    const unsigned slot = m / (unsigned)src.n_per_ray;
                    sdf_out[(size_t)slot * out_stride + (m - slot * (unsigned)src.n_per_ray)] = sdf;
                }
            }
        }
    }
    wait_glds();
}

}  // namespace f16x1

int sdf_f16x1_ref(const float* blob, const PointSrc& s, float R_bg, float* out, int out_stride, hipStream_t st);      // mlp_chain_f16x1.hip

// Precision 5's launcher (mlp_chain.hip::sdf_query).  NERFART_K2_F16X1=ref selects the k-step-outer kernel; read at every call, so that one process
// can run both (tests/test_gpu_k2_tile_outer.py).
int sdf_f16x1(const float* blob, const PointSrc& s, float R_bg, float* out, int out_stride, hipStream_t st) {
    const char* e = std::getenv("NERFART_K2_F16X1");
    if (e != nullptr && e[0] == 'r') return sdf_f16x1_ref(blob, s, R_bg, out, out_stride, st);
    return f16x1::launch_chain(0, (long long)s.M, f16x1::k_sdf_only_to, (s.M + 255u) / 256u, st, blob, s, R_bg, out, out_stride);
}

}  // namespace nerfart
