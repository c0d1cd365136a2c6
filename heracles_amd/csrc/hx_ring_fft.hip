// hx_ring_fft.hip -- ring Fourier stage of the HEALPix transforms (step 1 of the pipeline in hx_sht_common.h): the sub-DFT
// kernels of both directions, the Bluestein filter tables and the classification of a pixel-weight array.  This file alone knows
// which kernel a ring pair runs on, with how many threads, how much LDS and how many work-groups (ring_class_* below): plan
// creation (ring_fft_plan_init) sorts the ring pairs into classes by these rules, the launcher sizes its launches by them.
#include <algorithm>
#include <type_traits>

#include "hx_sht_common.h"

// (measured and not kept, round 5: the ring spectra leaving with non-temporal stores -- profiles/r05_fft_cycles.txt)

namespace hx {
// Bluestein filter spectra, one block per ring pair whose sub-length is not a power of two
// and is the first ring with that length.  The spectrum H (bit-reversed order, as the forward passes leave it) is stored
// TRANSPOSED, bhat[j (M/16) + i] = H[16 i + j]: in the ring kernel the thread that owns elements 16 i .. 16 i + 15 after the
// last forward pass multiplies them in registers, and for a fixed j consecutive threads then read consecutive entries
// (M < 16 -- the ring of 12 pixels -- keeps the plain order).
__global__ __launch_bounds__(512) void k_init_bhat(PlanDev P, const int *__restrict__ rp_list,
                                                   double2 *__restrict__ bhat)
{
    extern __shared__ double2 buf[];
    const int rp = rp_list[blockIdx.x];
    const int n = P.nsub[rp];
    const int M = fft_size_for(n);
    for (int j = threadIdx.x; j < lds_fft_slots(M); j += blockDim.x) buf[j] = make_double2(0.0, 0.0);
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double2 c = expipi((double)chirp_num(j, n) / (double)n);
        buf[lds_slot(j)] = c;
        if (j) buf[lds_slot(M - j)] = c;
    }
    __syncthreads();
    lds_fft_dif(buf, M, P.tw, P.twN);
    double2 *out = bhat + P.bhat_off[rp];
    for (int e = threadIdx.x; e < M; e += blockDim.x) out[M >= 16 ? (e & 15) * (M >> 4) + (e >> 4) : e] = buf[lds_slot(e)];
}

// =====================================================================================
// 1. ring Fourier stage: sub-DFTs in LDS
// =====================================================================================
// MODE 0: input = real maps (N ring -> real part, S ring -> imaginary part)
// MODE 1: input = complex spectrum Zc[c][ny-layout natural order] (synthesis: conj trick)
//
// A work item is ONE of the four length-n sub-DFTs X[4k + r] of a (ring pair, component): the group reads the 4n packed
// pixels z_q[j] = z[j + q n], forms t_r[j] = sum_q z_q[j] (-i)^(q r) on the fly and runs one transform in a padded LDS buffer,
// M / 16 threads, one radix-16 butterfly each per pass.  The four items of a ring pair are dealt to four work-groups of the
// SAME XCD that run at the same time (items are numbered xcd-minor, groups are persistent and walk items b, b + G, ...), so
// the pixels come from HBM once and from that XCD's L2 three more times -- and no thread has to keep a ring's pixels in
// registers across four transforms, which is what held the first version at one wave per SIMD with every latency exposed
// (256 registers of pixels beside the butterfly).  A transform is 3-4 LDS round trips (fused radix-8 / radix-16 passes); a
// Bluestein convolution fuses the last forward pass, the filter and the first inverse pass in registers (they work on the
// same 16 consecutive elements): 5-7 round trips for what were 13-15 with radix-4 passes and a filter pass of its own.  The
// filter values of a thread's butterfly are requested before the forward passes.  Every phase factor exp(-i pi q / 2n) (load
// phase, Bluestein chirps) is hi[q >> 6] lo[q & 63] from two small tables built per item in LDS: (4n / 64 + 65) sincos per
// item instead of one per pixel.
__host__ __device__ inline int ring_ph_hi(int M) { return (4 * M) / 64 + 1; }  // entries of the coarse phase table: q >> 6 for q < 4n, n <= M
constexpr int RING_NTMAX = 512;  // threads per group: M / 16 (one radix-16 butterfly per thread and pass), 64 at least
constexpr int RING_FB = 8;       // values of j per thread whose pixel loads are in flight together (64 loads)

// WSYM (MODE 0): the pixel-weight array has the symmetry of healpy's full weights -- it repeats over the four quadrants of a ring
// and from the northern to the southern ring of a pair -- so ONE weight per pixel pair of the first quadrant is read instead of
// eight.  Whether an array has that symmetry is found once per call of the C ABI (k_pixw_symmetry, one read of the array and a
// 4-byte read-back before anything else of the call is queued).  A template parameter, because a second run-time branch inside
// the batches of loads splits them (17.2 instead of 14.0 ms per 8 components even without weights); "weights or none" stays the
// run-time test it was (as a compile-time constant the 64 loads of the generic path are issued together: 256 registers, 34 spilled).
template <int MODE, bool WSYM = false>
__global__ __launch_bounds__(RING_NTMAX) void k_ring_subdft(PlanDev P, const RingDesc *__restrict__ desc, int nrings, int nb, int Mclass,
                                                            const double *__restrict__ maps,
                                                            const double *__restrict__ pixw,
                                                            const double2 *__restrict__ zin,
                                                            double2 *__restrict__ Y, double *__restrict__ pixout = nullptr,
                                                            const double *__restrict__ ref = nullptr)
{
    extern __shared__ double2 buf[];  // the padded transform buffer of the class's M, then the phase tables (4 M / 64 + 1 and 64 entries)
    __shared__ double2 tw_hi[TW_HI_MAX], tw_lo[64];
    double2 *ph_hi = buf + lds_fft_slots(Mclass), *ph_lo = ph_hi + ring_ph_hi(Mclass);
    const int nt = blockDim.x;
    const int nitems = ((nrings + 7) >> 3) * nb * 32;  // sets of 8 ring pairs (one per XCD) x components x 4 sub-DFTs
    const TwFactored twf = load_tw_factored(tw_hi, tw_lo, P.tw, P.twN);  // visible after the first barrier below
    int tid = threadIdx.x;
    // What an item needs to know about its ring pair is ONE 32-byte record (RingDesc; it was rp_list[ring], then P.nsub / startN / startS /
    // bhat_off [rp]: two dependent trips to memory in front of the pixel loads, a third one -- cycle accounting, profiles/r04_fft_cycles.txt:
    // "load + tables" 24k cycles per item whatever the length of its ring), and the record of the NEXT item is requested behind the first
    // batch of pixel loads of this one -- by a vector load with the same address in every lane (a scalar load would make the first
    // lgkmcnt(0) of the item wait for it) -- and moved to scalars after the fill, when it has long landed.
    auto ring_of = [&](int item) __attribute__((always_inline)) { return ((item >> 5) / nb) * 8 + (item & 7); };
    RingDesc cur = RingDesc{0, 0, 0, 1, 0};
    if ((int)blockIdx.x < nitems && ring_of(blockIdx.x) < nrings) cur = desc[ring_of(blockIdx.x)];
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        // item = 8 (4 s + r) + x: sub-DFT r of set s on XCD x -- the four r of a (ring pair, component) in four groups of that XCD,
        // side by side in time.  Set s = (ring set s / nb, component s % nb): an XCD walks the COMPONENTS of one ring pair before it
        // moves to its next ring pair, so that the pair's pixel weights come from HBM once and from that XCD's L2 for every other
        // component (component-major sets re-read the 1.6 GB weight array per component: +34 ms per step of the bench)
        const int r = (item >> 3) & 3, set = item >> 5;
        const int ring = ring_of(item), c = set % nb;
        const int itn = item + gridDim.x, ringn = itn < nitems ? ring_of(itn) : nrings;
        const bool nextv = ringn < nrings;
        if (ring >= nrings) {  // padding of the last set of 8 ring pairs
            if (nextv) cur = desc[ringn];
            continue;
        }
        const int n = cur.n;
        const long long sN = cur.sN, sS = cur.sS;
        const int M = fft_size_for(n), MP = lds_fft_slots(M);
        const bool blu = M != n;
        const int p = ilog2(M);
        const double2 *bh = P.bhat + cur.bhat_off;
        const double inv = 1.0 / M, inv4n = 0.25 / (double)n;
        // the thread index goes through an empty asm statement per item, so that what derives from it (LDS addresses, pixel
        // offsets) is set up per item instead of being hoisted out of this loop and kept in registers across the passes
        asm volatile("; item" : "+v"(tid));
        // ---- pixels.  RING_FB values of j at a time: all their loads (8 per j) are issued before the first is used -- one trip
        // to L2 / HBM per batch instead of one per j (out-of-range j read pixel 0 of the ring and write the spare slot of the
        // buffer; a missing southern ring (the equator) reads the northern one and selects 0).  The first batch is requested
        // before the phase tables are built, whose sincospi then cover part of its way ----
        const bool haveS = sS >= 0, odd = r & 1, pw = MODE == 0 && !WSYM && pixw != nullptr;
        constexpr bool wsym = MODE == 0 && WSYM;
        const double sg = (r & 2) ? -1.0 : 1.0;
        const double *mpN = maps + (long long)c * P.npix + sN, *mpS = maps + (long long)c * P.npix + (haveS ? sS : sN);
        const double *pwN = pixw + sN, *pwS = pixw + (haveS ? sS : sN);
        const double2 *zp = zin + (long long)c * P.ny + sN;
        double2 z[RING_FB][4];
        // A thread takes PAIRS of neighbouring j (j = 2 p, 2 p + 1, p = tid + k nt): one 16-byte load per ring, segment q and pair
        // instead of two 8-byte ones -- with pixel weights a batch is 64 loads, not 128 (the fill is bound by the number of load
        // instructions in flight, not by bytes).  An odd n leaves a last pair of one element: it reads the pair before it and
        // shifts (the segment [q n, (q + 1) n) is followed by the next one -- or, for q = 3, by the next ring, which the last
        // ring of the map does not have).
        struct __attribute__((aligned(8))) Pair { double x, y; };
        // A batch is REQUESTED here and FINISHED (pixel weights of the symmetric kind, the odd-n tail, the missing southern ring) where the
        // fill uses it: z[u][q], z[u + 1][q] hold the raw northern and southern pair until then.  Finished at the load -- as it was
        // since the weights came into the path -- every product needs its operand at once and hipcc issued two loads, s_waitcnt vmcnt(0),
        // two loads, ...: sixteen trips to memory one after the other, 23k of an item's 57-75k cycles whatever the length of its ring
        // (profiles/r04_fft_cycles.txt).  (Generic weight arrays keep that form: their raw values would need another 128 registers.)
        Pair wsy[RING_FB / 2];
        auto load_batch_t = [&](auto WIDEC, int u0) __attribute__((always_inline)) {
            constexpr bool WIDE = decltype(WIDEC)::value;
#pragma unroll
            for (int u = 0; u < RING_FB; u += 2) {
                const int j = 2 * (tid + ((u0 + u) >> 1) * nt);      // first j of the pair; the batch covers j < (u0 + RING_FB) nt
                const bool tail = WIDE && j == n - 1;                // (n = 1: the scalar path below)
                const int jj = tail ? n - 2 : (j + 1 < n ? j : 0);
                wsy[u >> 1] = Pair{1.0, 1.0};
                if (MODE == 0 && wsym && WIDE) wsy[u >> 1] = *reinterpret_cast<const Pair *>(pwN + jj);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = jj + q * n;
                    if (MODE == 0) {
                        Pair fn, fs;
                        if (WIDE) {
                            fn = *reinterpret_cast<const Pair *>(mpN + i);
                            fs = *reinterpret_cast<const Pair *>(mpS + i);
                            if (!wsym && pw) {
                                const Pair wn = *reinterpret_cast<const Pair *>(pwN + i), ws = *reinterpret_cast<const Pair *>(pwS + i);
                                fn.x *= wn.x; fn.y *= wn.y; fs.x *= ws.x; fs.y *= ws.y;
                            }
                            z[u][q] = make_double2(fn.x, fn.y);      // raw: finish_batch
                            z[u + 1][q] = make_double2(fs.x, fs.y);
                        } else {
                            fn.x = fn.y = mpN[q]; fs.x = fs.y = mpS[q];
                            if (pw || wsym) { fn.x *= pwN[q]; fs.x *= pwS[q]; fn.y = fn.x; fs.y = fs.x; }
                            z[u][q] = make_double2(fn.x, haveS ? fs.x : 0.0);
                            z[u + 1][q] = make_double2(fn.y, haveS ? fs.y : 0.0);
                        }
                    } else {
                        const int i0 = (j < n ? j : 0) + q * n, i1 = (j + 1 < n ? j + 1 : 0) + q * n;
                        z[u][q] = zp[i0];
                        z[u + 1][q] = zp[i1];
                    }
                }
            }
        };
        auto load_batch = [&](int u0) __attribute__((always_inline)) {
            if (n >= 2) load_batch_t(std::true_type{}, u0);
            else load_batch_t(std::false_type{}, u0);
        };
        // raw pairs -> the values of j and j + 1: (north, south) each
        auto finish_batch = [&](int u0) __attribute__((always_inline)) {
            if (MODE != 0 || n < 2) return;
#pragma unroll
            for (int u = 0; u < RING_FB; u += 2) {
                const int j = 2 * (tid + ((u0 + u) >> 1) * nt);
                const bool tail = j == n - 1;
                const Pair w = wsy[u >> 1];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double2 rn = z[u][q], rs = z[u + 1][q];
                    const double nx = wsym ? rn.x * w.x : rn.x, ny = wsym ? rn.y * w.y : rn.y;
                    const double sx = wsym ? rs.x * w.x : rs.x, sy = wsym ? rs.y * w.y : rs.y;
                    z[u][q] = make_double2(tail ? ny : nx, haveS ? (tail ? sy : sx) : 0.0);
                    z[u + 1][q] = make_double2(ny, haveS ? sy : 0.0);
                }
            }
        };
        load_batch(0);
        int4 nd0 = make_int4(0, 0, 0, 0), nd1 = nd0;  // the next item's record (see above)
        if (nextv) {
            const int4 *dp = reinterpret_cast<const int4 *>(desc + ringn) + (tid >> 30);
            nd0 = dp[0];
            nd1 = dp[1];
        }
        // (work-group barriers that wait for this wave's LDS traffic only: __syncthreads() would wait for the pixel loads too)
        auto lds_barrier = []() __attribute__((always_inline)) {
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
            __builtin_amdgcn_s_barrier();
        };
        lds_barrier();  // the previous item's last readers of the phase tables and of the buffer
        for (int a = tid; a <= (4 * n) >> 6; a += nt) ph_hi[a] = expipi(-(double)(a << 6) / (2.0 * n));
        if (tid < 64) ph_lo[tid] = expipi(-(double)tid / (2.0 * n));
        lds_barrier();
        auto phase = [&](unsigned q) __attribute__((always_inline)) {  // exp(-i pi q / 2n), q < 4n
            return cmul(ph_hi[q >> 6], ph_lo[q & 63]);
        };
        // ---- fill: t_r[j] x load phase.  t_r = (a, c)[r & 1] +- (b, d)[r & 1] with a = z0 + z2, b = z1 + z3, c = z0 - z2,
        // d = -i (z1 - z3) ----
        {
            for (int u0 = 0;;) {
                finish_batch(u0);
#pragma unroll
                for (int u = 0; u < RING_FB; ++u) {
                    const int j = 2 * (tid + ((u0 + u) >> 1) * nt) + (u & 1);  // the pairs of load_batch
                    const double2 e0 = odd ? csub(z[u][0], z[u][2]) : cadd(z[u][0], z[u][2]);
                    const double2 e1 = odd ? mul_mi(csub(z[u][1], z[u][3])) : cadd(z[u][1], z[u][3]);
                    const double2 t = make_double2(fma(sg, e1.x, e0.x), fma(sg, e1.y, e0.y));
                    // (j r + 2 j^2 [Bluestein]) mod 4n = load_phase_num(j, r, n, blu); j < 2^14: 32 bits hold it
                    const unsigned jc = j < n ? j : 0;
                    const unsigned qn = blu ? mod_by_inv(jc * (unsigned)r + 2u * jc * jc, 4u * (unsigned)n, inv4n) : jc * (unsigned)r;  // (j r < 4n as it is)
                    buf[j < n ? lds_slot(j) : MP - 1] = cmul(t, phase(qn));
                }
                u0 += RING_FB;
                if (u0 * nt >= n) break;
                load_batch(u0);
            }
            if (blu)
                for (int j = n + tid; j < M; j += nt) buf[lds_slot(j)] = make_double2(0.0, 0.0);  // Bluestein padding
        }
        __syncthreads();
        if (nextv) {
            auto sc = [](int v) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(v); };
            cur.sN = ((long long)sc(nd0.y) << 32) | (unsigned)sc(nd0.x);
            cur.sS = ((long long)sc(nd0.w) << 32) | (unsigned)sc(nd0.z);
            cur.bhat_off = ((long long)sc(nd1.y) << 32) | (unsigned)sc(nd1.x);
            cur.n = sc(nd1.z);
            cur.rp = sc(nd1.w);
        }
        double2 *out = Y + (long long)c * P.ny + sN + (long long)r * n;
        // MODE 1 with `pixout` (synthesis, round 6): the value of bin k of sub-DFT r IS the pixel pair 4 k + r of the two rings --
        // Y_r[k] = conj(z[4 k + r]), f_N = Re, f_S = -Im -- so it goes straight to the maps (or, with `ref`, the residual ref - synthesised of
        // a Jacobi iteration) instead of through Y and a scatter pass of its own (16 B written + 16 B read + 16 B written per pixel pair
        // before; the four items of a ring pair run side by side on one XCD, whose L2 merges their interleaved 8-byte stores)
        double *pxN = nullptr, *pxS = nullptr;
        const double *rfN = nullptr, *rfS = nullptr;
        if (MODE == 1 && pixout) {
            pxN = pixout + (long long)c * P.npix + sN + r;
            pxS = pixout + (long long)c * P.npix + (haveS ? sS : sN) + r;
            if (ref) { rfN = ref + (long long)c * P.npix + sN + r; rfS = ref + (long long)c * P.npix + (haveS ? sS : sN) + r; }
        }
        // MODE 0: bins 4 k + r that no order m <= lmax falls on (neither as m nor as 4n - m) are not written: a ring of 4n > 2 lmax + 1
        // pixels leaves lmax < bin < 4n - lmax out -- a quarter of the belt's stores at nside 4096 / lmax 6144, half at nside 8192 / lmax 8000
        // (the read-out is a burst of stores into the in-order memory pipeline: what the item waits for at its end)
        const int kdrop0 = MODE == 0 ? (P.lmax - r) / 4 + 1 : n, kdrop1 = (4 * n - P.lmax - r + 3) / 4;
        auto emit = [&](int k, double2 v) __attribute__((always_inline)) {
            if (MODE == 0 && k >= kdrop0 && k < kdrop1) return;
            if (MODE == 1 && pxN) {
                double fn = v.x, fs = -v.y;
                if (rfN) { fn = rfN[4 * k] - fn; fs = rfS[4 * k] - fs; }
                pxN[4 * k] = fn;
                if (haveS) pxS[4 * k] = fs;
            } else {
                out[k] = v;
            }
        };
        if (!blu) {
            lds_fft_dif(buf, M, twf, P.twN);
            for (int k = tid; k < n; k += nt) emit(k, buf[lds_slot(bitrev(k, p))]);
            continue;
        }
        if (M >= 16) {
            // filter values of this thread's first butterfly of the fused pass: requested before the forward passes, which
            // cover the trip to L2 / HBM (waited for inside the butterfly loop it cost 13 000 cycles per butterfly)
            double2 bq[16];
            const int nbf = M >> 4;
#pragma unroll
            for (int j = 0; j < 16; ++j) bq[j] = bh[j * nbf + (tid < nbf ? tid : 0)];
            lds_fft_dif(buf, M, twf, P.twN, tid, nt, true);
            // last forward pass (h = 1: no twiddles), filter, first inverse pass on the thread's 16 consecutive elements
#pragma unroll 1
            for (int i = tid; i < nbf; i += nt) {
                double2 x[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = buf[lds_slot(16 * i) + j];
                dif_regs<4>(x);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    x[j] = cmul(x[j], bq[j]);
                }
                if (i + nt < nbf) {  // (groups of fewer than M / 16 threads: tiny rings only)
#pragma unroll
                    for (int j = 0; j < 16; ++j) bq[j] = bh[j * nbf + i + nt];
                }
                dit_inv_regs<4>(x);
#pragma unroll
                for (int j = 0; j < 16; ++j) buf[lds_slot(16 * i) + j] = x[j];
            }
            __syncthreads();
            lds_fft_dit_inv(buf, M, twf, P.twN, tid, nt, true);
        } else {
            lds_fft_dif(buf, M, twf, P.twN, tid, nt);
            for (int j = tid; j < M; j += nt) buf[lds_slot(j)] = cmul(buf[lds_slot(j)], bh[j]);
            __syncthreads();
            lds_fft_dit_inv(buf, M, twf, P.twN, tid, nt);
        }
        for (int k = tid; k < n; k += nt)  // chirp exp(-i pi k^2 / n)
            emit(k, cscale(cmul(buf[lds_slot(k)], phase(2u * mod_by_inv((unsigned)k * (unsigned)k, 2u * (unsigned)n, 2.0 * inv4n))), inv));
    }
}

// =====================================================================================
// 1a. rings of 4 x 2^k pixels (the equatorial belt, and the cap rings with n = 2^k): plain FFTs, no Bluestein convolution.  The
//     four work items of a (ring pair, component) of the kernel above each read ALL of the pair's pixels (and pixel weights): 3 of
//     the 4 reads come from L2, but the belt is 5120 of the 8192 ring pairs at nside 4096 and its items spend 60 % (without weights)
//     to 80 % (with) of their cycles waiting for those reads (tools/fft_ablate.sh 32: load + fill 102k of 173k / 275k of 337k
//     cycles per ring pair and component) -- 515 GB through the L2s per step of the bench.  Here a work item is TWO sub-DFTs,
//     r and r + 2: they are the sum and the difference of the same two combinations of the four segments
//         t_r = e0 + e1,  t_{r+2} = e0 - e1,   e0 = z0 +- z2,  e1 = z1 +- z3 (x -i for odd r),
//     so one read of the pixels fills two LDS buffers, and the two halves of the work-group (M / 16 threads each) run one
//     transform each: half the reads.  Two 4096-point buffers are 139 KiB: one group of 512 threads per CU.
// =====================================================================================
template <int MODE, bool WSYM = false>
__global__ __launch_bounds__(RING_NTMAX) void k_ring_pairfft(PlanDev P, const RingDesc *__restrict__ desc, int nrings, int nb, int M,
                                                             const double *__restrict__ maps, const double *__restrict__ pixw,
                                                             const double2 *__restrict__ zin, double2 *__restrict__ Y,
                                                             double *__restrict__ pixout = nullptr, const double *__restrict__ ref = nullptr)
{
    extern __shared__ double2 buf[];  // two padded buffers of M points, then the phase tables (4 M / 64 + 1 and 64 entries)
    __shared__ double2 tw_hi[TW_HI_MAX], tw_lo[64];
    const int MP = lds_fft_slots(M), n = M, p = ilog2(M);
    double2 *ph_hi = buf + 2 * MP, *ph_lo = ph_hi + ring_ph_hi(M);
    const int nt = blockDim.x, nh = nt >> 1;  // threads of the group / of one transform
    // Two work items per (ring pair, component), one per round, side by side on one XCD.  (Measured and not kept: one work item that runs
    // both rounds from ONE read, its pixels -- 128 registers -- kept across the transforms: 46 registers spilled, 18.9 vs 19.4 ms per 8
    // components with pixel weights, 15.1 vs 14.3 without, same device.)
    const int nitems = ((nrings + 7) >> 3) * nb * 16;
    const TwFactored twf = load_tw_factored(tw_hi, tw_lo, P.tw, P.twN);
    int tid = threadIdx.x;
    // the phase tables depend on n = M only: built once per group
    for (int a = tid; a <= (4 * n) >> 6; a += nt) ph_hi[a] = expipi(-(double)(a << 6) / (2.0 * n));
    if (tid < 64) ph_lo[tid] = expipi(-(double)tid / (2.0 * n));
    __syncthreads();
    auto phase = [&](unsigned q) __attribute__((always_inline)) { return cmul(ph_hi[q >> 6], ph_lo[q & 63]); };  // exp(-i pi q / 2n), q < 4n
    // (the record of the next item's ring pair is requested behind this item's pixel loads: see k_ring_subdft)
    auto ring_of = [&](int item) __attribute__((always_inline)) { return ((item >> 4) / nb) * 8 + (item & 7); };
    auto comp_of = [&](int item) __attribute__((always_inline)) { return (item >> 4) % nb; };
    RingDesc cur = RingDesc{0, 0, 0, 1, 0};
    if ((int)blockIdx.x < nitems && ring_of(blockIdx.x) < nrings) cur = desc[ring_of(blockIdx.x)];
    // Pixels: pairs of neighbouring j: 2 (tid + k nt), k < 4 (n / 2 pairs over nt = n / 8 threads, or 128 threads for n <= 1024).  A batch is
    // REQUESTED raw -- z[u][q], z[u + 1][q] hold the northern and the southern pair, the symmetric weight pair sits beside them -- and
    // FINISHED where the fill uses it (k_ring_subdft).  The FIRST HALF of the NEXT item's batch (u < 4: 72 registers) is requested
    // behind this item's fill and lands under its transforms and read-out -- the radix-16 passes (134 registers) leave room for half a
    // batch, not for a whole one; the second half goes out at the start of the item and lands under the fill of the first.  (An item
    // used to wait 21k of its 52k cycles for its one batch with nothing to cover it: one work-group per CU.)
    struct __attribute__((aligned(8))) Pair { double x, y; };
    double2 z[RING_FB][4];
    Pair wsy[RING_FB / 2];
    const bool pw = MODE == 0 && !WSYM && pixw != nullptr;
    constexpr bool wsym = MODE == 0 && WSYM;
    auto request = [&](auto U0C, const RingDesc &d, int c) __attribute__((always_inline)) {
        constexpr int U0 = decltype(U0C)::value;
        const bool hS = d.sS >= 0;
        const double *mpN = maps + (long long)c * P.npix + d.sN, *mpS = maps + (long long)c * P.npix + (hS ? d.sS : d.sN);
        const double *pwN = pixw + d.sN, *pwS = pixw + (hS ? d.sS : d.sN);
        const double2 *zp = zin + (long long)c * P.ny + d.sN;
#pragma unroll
        for (int u = U0; u < U0 + RING_FB / 2; u += 2) {
            const int j = 2 * (tid + (u >> 1) * nt), jj = j + 1 < n ? j : 0;
            wsy[u >> 1] = Pair{1.0, 1.0};
            if (MODE == 0 && wsym) wsy[u >> 1] = *reinterpret_cast<const Pair *>(pwN + jj);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = jj + q * n;
                if (MODE == 0) {
                    Pair fn = *reinterpret_cast<const Pair *>(mpN + i), fs = *reinterpret_cast<const Pair *>(mpS + i);
                    if (!wsym && pw) {  // (generic weight arrays: applied at the load -- their raw values would need another 128 registers)
                        const Pair wn = *reinterpret_cast<const Pair *>(pwN + i), ws = *reinterpret_cast<const Pair *>(pwS + i);
                        fn.x *= wn.x; fn.y *= wn.y; fs.x *= ws.x; fs.y *= ws.y;
                    }
                    z[u][q] = make_double2(fn.x, fn.y);
                    z[u + 1][q] = make_double2(fs.x, fs.y);
                } else {
                    z[u][q] = zp[i];
                    z[u + 1][q] = zp[i + 1];
                }
            }
        }
    };
    auto finish = [&](bool hS) __attribute__((always_inline)) {
        if (MODE != 0) return;
#pragma unroll
        for (int u = 0; u < RING_FB; u += 2) {
            const Pair w = wsy[u >> 1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double2 rn = z[u][q], rs = z[u + 1][q];
                const double nx = wsym ? rn.x * w.x : rn.x, ny = wsym ? rn.y * w.y : rn.y;
                const double sx = wsym ? rs.x * w.x : rs.x, sy = wsym ? rs.y * w.y : rs.y;
                z[u][q] = make_double2(nx, hS ? sx : 0.0);
                z[u + 1][q] = make_double2(ny, hS ? sy : 0.0);
            }
        }
    };
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, RING_FB / 2>;
    bool have_half = false;  // the first half of this item's batch was requested by the item before it
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        // one round per item: item = 8 (2 s + rpair) + x -- the two items of set s = (ring set s / nb, component s % nb) on XCD x
        const int rpair = (item >> 3) & 1;  // round 0 = sub-DFTs 0 and 2, round 1 = sub-DFTs 1 and 3
        const int ring = ring_of(item), c = comp_of(item);
        const int itn = item + gridDim.x, ringn = itn < nitems ? ring_of(itn) : nrings;
        const bool nextv = ringn < nrings;
        if (ring >= nrings) {
            if (nextv) cur = desc[ringn];
            have_half = false;
            continue;
        }
        const long long sN = cur.sN, sS = cur.sS;
        asm volatile("; item" : "+v"(tid));
        const bool haveS = sS >= 0;
        if (!have_half) request(H0{}, cur, c);
        request(H1{}, cur, c);
        int4 nd0 = make_int4(0, 0, 0, 0);
        if (nextv) nd0 = *(reinterpret_cast<const int4 *>(desc + ringn) + (tid >> 30));
        {
        // (the previous round's read-out has to be over before the buffers are filled again)
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
        finish(haveS);
#pragma unroll
        for (int u = 0; u < RING_FB; ++u) {
            const int j = 2 * (tid + (u >> 1) * nt) + (u & 1);
            if (j >= n) continue;
            const double2 e0 = rpair ? csub(z[u][0], z[u][2]) : cadd(z[u][0], z[u][2]);
            const double2 e1 = rpair ? mul_mi(csub(z[u][1], z[u][3])) : cadd(z[u][1], z[u][3]);
            // load phases exp(-i pi j r / 2n) of r = rpair and r + 2: j < n and r <= 3, so j r < 4n needs no reduction, and r = 0 no phase at all
            const double2 t0 = cadd(e0, e1);
            buf[lds_slot(j)] = rpair ? cmul(t0, phase((unsigned)j)) : t0;
            buf[MP + lds_slot(j)] = cmul(csub(e0, e1), phase((unsigned)j * (unsigned)(rpair + 2)));
        }
        __syncthreads();
        // the next item's record: taken HERE, in front of this item's stores -- waited for behind them (their number is not known to
        // the compiler) it is s_waitcnt vmcnt(0), and the next item's loads are issued when the last store has been acknowledged
        have_half = false;
        if (nextv) {
            cur.sN = ((long long)__builtin_amdgcn_readfirstlane(nd0.y) << 32) | (unsigned)__builtin_amdgcn_readfirstlane(nd0.x);
            cur.sS = ((long long)__builtin_amdgcn_readfirstlane(nd0.w) << 32) | (unsigned)__builtin_amdgcn_readfirstlane(nd0.z);
            request(H0{}, cur, comp_of(itn));  // (z is free behind the last fill of the item)
            have_half = true;
        }
        const int half = tid >= nh ? 1 : 0, gt = tid - half * nh;
        double2 *bh = buf + half * MP;
        lds_fft_dif(bh, M, twf, P.twN, gt, nh);
        const int r = rpair + 2 * half;
        if (MODE == 1 && pixout) {  // straight to the pixels 4 k + r of the two rings, or to the residual (see k_ring_subdft)
            double *pxN = pixout + (long long)c * P.npix + sN + r, *pxS = pixout + (long long)c * P.npix + (haveS ? sS : sN) + r;
            if (ref) {
                const double *rfN = ref + (long long)c * P.npix + sN + r, *rfS = ref + (long long)c * P.npix + (haveS ? sS : sN) + r;
                for (int k = gt; k < n; k += nh) {
                    const double2 v = bh[lds_slot(bitrev(k, p))];
                    pxN[4 * k] = rfN[4 * k] - v.x;
                    if (haveS) pxS[4 * k] = rfS[4 * k] + v.y;
                }
            } else {
                for (int k = gt; k < n; k += nh) {
                    const double2 v = bh[lds_slot(bitrev(k, p))];
                    pxN[4 * k] = v.x;
                    if (haveS) pxS[4 * k] = -v.y;
                }
            }
        } else {
            double2 *out = Y + (long long)c * P.ny + sN + (long long)r * n;
            // (MODE 0: bins between lmax and 4n - lmax are not written, see k_ring_subdft)
            const int kdrop0 = MODE == 0 ? (P.lmax - r) / 4 + 1 : n, kdrop1 = (4 * n - P.lmax - r + 3) / 4;
            for (int k = gt; k < n; k += nh)
                if (k < kdrop0 || k >= kdrop1) *(out + k) = bh[lds_slot(bitrev(k, p))];
        }
        }
    }
}

// (Round 6, measured and not kept: the same work item with its two transforms run one after the other through ONE buffer by half as many threads, so
// that two independent groups fit a CU -- analysis 51.1 -> 50.6 ms per step, synthesis of ten fields 51.4 -> 56.1 ms: the item is bound by the issue of its
// vector instructions and by dependent LDS round trips, not by latency a second group could cover.  profiles/r06_pairseq_experiment.txt.)
// =====================================================================================
// 1b. rings whose Bluestein convolution does not fit LDS (nside 8192: cap rings with 4096 < n < 8192 need M = 16384 points
//     = 256 KiB): the length-M cyclic convolution as an EVEN and an ODD half of C = M / 2 points each
//         X[2k]   = FFT_C( x[j] + x[j + C] )[k],      X[2k+1] = FFT_C( (x[j] - x[j + C]) W_M^j )[k]         (forward, DIF)
//         y[j]    = IFFT_C(Y_even)[j] + W_M^-j IFFT_C(Y_odd)[j],   j < C                                      (inverse, DIT)
//     The input has n <= C non-zero points (x[j + C] = 0) and only y[0..n) is wanted, so each half is exactly the in-LDS
//     pipeline of the other rings (FFT_C -> filter -> IFFT_C) on one C-point buffer; the even half's result waits in
//     registers while the odd half runs.  The filter spectra are stored as [even bins | odd bins].
// =====================================================================================
constexpr int SPLIT_JMAX = 16;  // values of j per thread of the split kernels (n <= C = 16 x 512 threads at most; 512 threads: 256 registers for the radix-16 passes)

__global__ __launch_bounds__(512) void k_init_bhat_split(PlanDev P, const int *__restrict__ rp_list, int C,
                                                          double2 *__restrict__ bhat)
{
    extern __shared__ double2 buf[];
    const int rp = rp_list[blockIdx.x];
    const int n = P.nsub[rp], M = 2 * C;
    double2 *out = bhat + P.bhat_off[rp];
    // filter b[j] = chirp(j) for j < n, b[M - j] = chirp(j), 0 elsewhere; halves b0 = b[0..C), b1 = b[C..M)
    auto b_at = [&](int j) {  // 0 <= j < M
        const int jj = j < n ? j : (M - j < n ? M - j : -1);
        return jj < 0 ? make_double2(0.0, 0.0) : expipi((double)chirp_num(jj, n) / (double)n);
    };
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        for (int j = threadIdx.x; j < C; j += blockDim.x) {
            const double2 b0 = b_at(j), b1 = b_at(j + C);
            buf[lds_slot(j)] = half == 0 ? cadd(b0, b1) : cmul(csub(b0, b1), P.tw[j]);  // tw[j] = W_M^j (twN = M)
        }
        __syncthreads();
        lds_fft_dif(buf, C, P.tw, P.twN);
        for (int j = threadIdx.x; j < C; j += blockDim.x) out[half * C + j] = buf[lds_slot(j)];
    }
}

template <int MODE>
__global__ __launch_bounds__(512) void k_ring_subdft_split(PlanDev P, const int *__restrict__ rp_list, int C,
                                                            const double *__restrict__ maps, const double *__restrict__ pixw,
                                                            const double2 *__restrict__ zin, double2 *__restrict__ Y,
                                                            double *__restrict__ pixout = nullptr, const double *__restrict__ ref = nullptr)
{
    extern __shared__ double2 buf[];
    const int rp = rp_list[blockIdx.y];
    const int c = blockIdx.z;
    const int n = P.nsub[rp];
    const long long sN = P.startN[rp], sS = P.startS[rp];
    const int M = 2 * C;
    const bool plain = fft_size_for(n) == n;  // a power of two (n == C): one plain FFT, no convolution
    const double *mp = maps + (long long)c * P.npix;
    const double2 *zp = zin + (long long)c * P.ny + sN;
    const double2 *bh = P.bhat + (plain ? 0 : P.bhat_off[rp]);
    const double inv = 1.0 / M;
    __shared__ double2 tw_hi[TW_HI_MAX], tw_lo[64];
    const TwFactored twf = load_tw_factored(tw_hi, tw_lo, P.tw, P.twN);
    auto z_at = [&](int j, int q) {  // packed ring value z_q[j] = z[j + q n]
        if (MODE == 0) {
            const long long iN = sN + j + (long long)q * n;
            double fn = mp[iN];
            if (pixw) fn *= pixw[iN];
            double fs = 0.0;
            if (sS >= 0) {
                const long long iS = sS + j + (long long)q * n;
                fs = mp[iS];
                if (pixw) fs *= pixw[iS];
            }
            return make_double2(fn, fs);
        }
        return zp[j + (long long)q * n];
    };
    // Nothing is carried in registers across the transforms (round 6): until then the 16 input values a0[j] and the 16 results of the even
    // half sat in registers under the radix-16 passes -- 256 registers, 1 050 more in scratch (3.2 KB per lane), 35 ms for the cap rings of
    // two maps at nside 8192, two thirds of their ring stage.  Now the input of the odd half is formed again from the pixels (L2) and the
    // even half's result waits where it belongs -- in Y, or in the pixels -- for the odd half to be ADDED to it by the same thread.
    // (MODE 1 with pixout: bin k of sub-DFT r goes straight to the pixel pair 4 k + r of the two rings, see k_ring_subdft.)
    auto emit = [&](int r, int k, double2 v, bool add) __attribute__((always_inline)) {
        if (MODE == 1 && pixout) {
            const long long iN = (long long)c * P.npix + sN + 4 * k + r, iS = (long long)c * P.npix + sS + 4 * k + r;
            if (add) {  // (what is there is ref - first part, or the first part: subtract / add the second)
                pixout[iN] += ref ? -v.x : v.x;
                if (sS >= 0) pixout[iS] += ref ? v.y : -v.y;
            } else {
                double fn = v.x, fs = -v.y;
                if (ref) { fn = ref[iN] - fn; if (sS >= 0) fs = ref[iS] - fs; }
                pixout[iN] = fn;
                if (sS >= 0) pixout[iS] = fs;
            }
        } else {
            double2 *o = Y + (long long)c * P.ny + sN + (long long)r * n + k;
            *o = add ? cadd(*o, v) : v;
        }
    };
    // t_r[j] exp(-i pi (j r + 2 j^2 [Bluestein]) / 2n)
    auto input = [&](int r, int j) __attribute__((always_inline)) {
        const double2 t = dif4_combine(z_at(j, 0), z_at(j, 1), z_at(j, 2), z_at(j, 3), r);
        const unsigned qn = load_phase_num(j, r, n, !plain);
        return qn ? cmul(t, expipi(-(double)qn / (2.0 * n))) : t;
    };
    for (int r = 0; r < 4; ++r) {
        if (plain) {
            __syncthreads();
#pragma unroll 4
            for (int u = 0; u < SPLIT_JMAX; ++u) {
                const int j = threadIdx.x + u * blockDim.x;
                if (j < n) buf[lds_slot(j)] = input(r, j);
            }
            __syncthreads();
            lds_fft_dif(buf, n, twf, P.twN);
            const int pbits = ilog2(n);
            for (int k = threadIdx.x; k < n; k += blockDim.x) emit(r, k, buf[lds_slot(bitrev(k, pbits))], false);
            continue;
        }
        for (int half = 0; half < 2; ++half) {
            __syncthreads();  // the previous pass has been read out of buf
#pragma unroll 4
            for (int u = 0; u < SPLIT_JMAX; ++u) {
                const int j = threadIdx.x + u * blockDim.x;
                if (j < C) {
                    double2 v = make_double2(0.0, 0.0);
                    if (j < n) {
                        v = input(r, j);
                        if (half) v = cmul(v, twf[j]);
                    }
                    buf[lds_slot(j)] = v;
                }
            }
            __syncthreads();
            lds_fft_dif(buf, C, twf, P.twN);
            for (int j = threadIdx.x; j < C; j += blockDim.x) buf[lds_slot(j)] = cmul(buf[lds_slot(j)], bh[half * C + j]);
            __syncthreads();
            lds_fft_dit_inv(buf, C, twf, P.twN);
#pragma unroll 4
            for (int u = 0; u < SPLIT_JMAX; ++u) {
                const int k = threadIdx.x + u * blockDim.x;
                if (k < n) {
                    double2 y = buf[lds_slot(k)];
                    if (half) y = cmulc(y, twf[k]);  // W_M^-k y_odd[k]
                    emit(r, k, cscale(cmul(y, expipi(-(double)chirp_num(k, n) / (double)n)), inv), half != 0);
                }
            }
        }
    }
}

// flag stays != 0 if the weights of every ring pair repeat over its four quadrants and from its northern to its southern ring
// (bitwise): one read of the array, 0.4 ms at nside 4096 per call, against 8 weight loads per pixel pair in every ring kernel
__global__ __launch_bounds__(256) void k_pixw_symmetry(PlanDev P, const double *__restrict__ pixw, int *__restrict__ flag)
{
    const int rp = blockIdx.x, n = P.nsub[rp];
    const long long sN = P.startN[rp], sS = P.startS[rp];
    bool ok = true;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const double w = pixw[sN + j];
#pragma unroll
        for (int q = 1; q < 4; ++q) ok = ok && pixw[sN + j + (long long)q * n] == w;
        if (sS >= 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ok = ok && pixw[sS + j + (long long)q * n] == w;
        }
    }
    if (!ok) *flag = 0;
}

}  // namespace hx

using namespace hx;

// Longest FFT done in LDS (points; 8192 = 128 KiB of the CU's 160).  Lowering it (hx_set_max_lds_fft, a power of two >= 16)
// sends smaller rings through the split kernels -- the way the tests exercise them without an nside-8192 map.
static int g_lds_fft_cap = 8192;
extern "C" int hx_set_max_lds_fft(int points)
{
    if (points < 16 || points > 8192 || (points & (points - 1))) return fail(HX_ERR_ARG, "hx_set_max_lds_fft: a power of two in [16, 8192]");
    g_lds_fft_cap = points;
    return HX_OK;
}

// =====================================================================================
// the class of a ring pair: kernel, threads, LDS, work-groups
// =====================================================================================
// Dynamic LDS of a work-group at in-LDS FFT length M: the padded transform buffer -- two of them in k_ring_pairfft -- and the
// phase tables behind it (4 M / 64 + 1 and 64 entries).
static size_t ring_class_lds(int M, bool pair) { return ((pair ? 2 : 1) * (size_t)lds_fft_slots(M) + ring_ph_hi(M) + 64) * sizeof(double2); }

// k_ring_pairfft takes the plain 2^k rings whose two buffers fit LDS (4 KiB aside for the static twiddle tables)
static bool ring_class_is_pair(int n, int M, int cap) { return M == n && M >= 16 && M <= cap && ring_class_lds(M, true) + 4096 <= 160 * 1024; }

// What plan creation does for the ring Fourier stage: FFT classes, the records of their ring pairs, Bluestein filter spectra, and
// the LDS the kernels may ask for.  Called behind plan_tables (the filters are transformed with its twiddles: pl->tw, pl->twN).
int hx::ring_fft_plan_init(hx_plan *pl, const std::vector<int> &nsub, const std::vector<long long> &sN, const std::vector<long long> &sS)
{
    // in-LDS FFT length limit (8192 points = 128 KiB); Bluestein rings of twice that run as two halves (split kernels)
    const int cap = g_lds_fft_cap;
    // FFT-size classes: ring pairs grouped by in-LDS FFT length, longest rings first; rings beyond the limit form
    // the split class (M = 2 x cap)
    // (second key: 0 regular kernel; -1 plain 2^k rings whose two buffers fit LDS: the pair kernel)
    std::map<std::pair<int, int>, std::vector<int>> byM;
    bool plain_beyond_cap = false;
    for (int rp = pl->nrp - 1; rp >= 0; --rp) {
        const int M = fft_size_for(nsub[rp]);
        byM[{M, ring_class_is_pair(nsub[rp], M, cap) ? -1 : 0}].push_back(rp);
        plain_beyond_cap = plain_beyond_cap || (M > cap && M == nsub[rp]);
    }
    const int maxM = byM.rbegin()->first.first;
    if (maxM > 2 * cap || plain_beyond_cap) return fail(HX_ERR_UNSUPPORTED, "hx_plan_create: nside=%d needs an in-LDS FFT of %d points (limit %d, %d for Bluestein rings); unsupported", pl->nside, maxM, cap, 2 * cap);
    pl->fft_cap = cap;
    pl->lds_fft = (size_t)lds_fft_slots(std::min(maxM, cap)) * sizeof(double2);
    for (auto it = byM.rbegin(); it != byM.rend(); ++it) {
        pl->fft_classes.push_back({it->first.first, (int)pl->h_fft_rp_list.size(), (int)it->second.size(), it->first.second});  // M, first, count, big
        pl->h_fft_rp_list.insert(pl->h_fft_rp_list.end(), it->second.begin(), it->second.end());
    }
    HX_TRY(upload(pl->fft_rp_list, pl->h_fft_rp_list));
    // Bluestein tables: one spectrum per distinct non-power-of-two sub-length
    std::vector<long long> boff(pl->nrp, -1);
    std::vector<int> blu_list, blu_split;
    long long btot = 0;
    std::map<int, long long> off_of_n;
    for (int rp = 0; rp < pl->nrp; ++rp) {
        int n = nsub[rp], M = fft_size_for(n);
        if (M == n) continue;
        auto it = off_of_n.find(n);
        if (it == off_of_n.end()) {
            it = off_of_n.emplace(n, btot).first;
            btot += M;
            (M > cap ? blu_split : blu_list).push_back(rp);
        }
        boff[rp] = it->second;
    }
    HX_TRY(upload(pl->bhat_off, boff));
    std::vector<RingDesc> desc;
    for (int rp : pl->h_fft_rp_list) desc.push_back(RingDesc{sN[rp], sS[rp], boff[rp], nsub[rp], rp});
    HX_TRY(upload(pl->fft_desc, desc));
    HX_TRY(pl->bhat.alloc(sizeof(double2) * std::max<long long>(btot, 1)));
    // the LDS the kernels may ask for: 3 KiB of the 160 KiB are the static twiddle tables of the ring kernels
    const void *const init_kernels[] = {(const void *)k_init_bhat, (const void *)k_init_bhat_split};
    const void *const ring_kernels[] = {(const void *)k_ring_subdft<0, false>,  (const void *)k_ring_subdft<0, true>,  (const void *)k_ring_subdft<1, false>,
                                        (const void *)k_ring_pairfft<0, false>, (const void *)k_ring_pairfft<0, true>, (const void *)k_ring_pairfft<1, false>,
                                        (const void *)k_ring_subdft_split<0>,   (const void *)k_ring_subdft_split<1>};
    for (const void *k : init_kernels) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (const void *k : ring_kernels) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    HX_HIP(hipGetLastError());
    hipStream_t st = rt().stream;
    if (!blu_list.empty()) {
        DevBuf d_list;
        HX_TRY(upload(d_list, blu_list));
        hipLaunchKernelGGL(k_init_bhat, dim3((unsigned)blu_list.size()), dim3(512), pl->lds_fft, st, pl->dev(),
                           d_list.as<int>(), pl->bhat.as<double2>());
        (void)hipStreamSynchronize(st);
    }
    if (!blu_split.empty()) {
        DevBuf d_list;
        HX_TRY(upload(d_list, blu_split));
        hipLaunchKernelGGL(k_init_bhat_split, dim3((unsigned)blu_split.size()), dim3(std::min(512, std::max(64, cap / 16))), (size_t)lds_fft_slots(cap) * sizeof(double2), st,
                           pl->dev(), d_list.as<int>(), cap, pl->bhat.as<double2>());
        (void)hipStreamSynchronize(st);
    }
    return HX_OK;
}

// =====================================================================================
// launches
// =====================================================================================
// what the ring kernels read and write: real maps (x pixel weights) -> Y (MODE 0), or spectra zin -> pixels or, with ref, the
// residual ref - synthesised (MODE 1)
struct RingIO { const double *maps, *pixw; const double2 *zin; double2 *Y; double *pixout; const double *ref; };

// A class of k_ring_subdft (k = 1) or k_ring_pairfft (k = 2 transforms per group, half as many work items per set of 8 ring pairs
// x component).  M / 16 threads per transform (one radix-16 butterfly per thread and pass), 64 at least; persistent groups, as
// many as the CUs hold at once: LDS (the padded buffers, the phase tables behind them, 3 KiB of twiddle tables) and 8 waves per
// CU, so that every wave has 256 registers
template <auto KERNEL>
static void launch_ring_class(hx_plan *pl, const hx_plan::FftClass &c, int nb, const RingIO &io)
{
    const int k = c.big < 0 ? 2 : 1;
    const int threads = std::min(RING_NTMAX, k * std::max(64, c.M / 16));
    const size_t lds = ring_class_lds(c.M, k == 2);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(512 / threads, (160 * 1024) / (lds + 3 * 1024 + 256)));
    const long long items = ((long long)c.count + 7) / 8 * nb * (32 / k);
    const unsigned groups = (unsigned)std::min<long long>(items, (long long)rt().cus * per_cu);
    hipLaunchKernelGGL(KERNEL, dim3(groups), dim3(threads), lds, rt().stream, pl->dev(), pl->fft_desc.as<RingDesc>() + c.first, c.count, nb, c.M, io.maps, io.pixw, io.zin, io.Y, io.pixout, io.ref);
}

// One launch per FFT-size class, so that every class gets the LDS it needs and no more
// (a 4096-point ring must not reserve the 128 KiB of an 8192-point Bluestein ring).
template <int MODE, bool WSYM>
static int launch_subdft_classes(hx_plan *pl, int nb, const RingIO &io, int rp_lo = 0, int rp_hi = 0x7fffffff)
{
    for (const auto &cls : pl->fft_classes) {
        // the ring pairs of the class that lie in [rp_lo, rp_hi): its list is in descending order, so they are one run of it
        hx_plan::FftClass c = cls;
        if (rp_lo > 0 || rp_hi < pl->nrp) {
            const int *b = pl->h_fft_rp_list.data() + cls.first, *e = b + cls.count;
            const int *x = std::lower_bound(b, e, rp_hi, [](int rp, int lim) { return rp >= lim; });  // first rp < rp_hi
            const int *y = std::lower_bound(b, e, rp_lo, [](int rp, int lim) { return rp >= lim; });  // first rp < rp_lo
            c.first = cls.first + (int)(x - b);
            c.count = (int)(y - x);
            if (c.count <= 0) continue;
        }
        if (c.big < 0)  // plain 2^k rings: two sub-DFTs per work item
            launch_ring_class<k_ring_pairfft<MODE, WSYM>>(pl, c, nb, io);
        else if (c.M > pl->fft_cap) {  // Bluestein convolution of 2 x cap points in two halves
            const int C = pl->fft_cap, threads = std::min(512, std::max(64, C / SPLIT_JMAX));
            hipLaunchKernelGGL(k_ring_subdft_split<MODE>, dim3(1, c.count, nb), dim3(threads), (size_t)lds_fft_slots(C) * sizeof(double2), rt().stream,
                               pl->dev(), pl->fft_rp_list.as<int>() + c.first, C, io.maps, io.pixw, io.zin, io.Y, io.pixout, io.ref);
        } else
            launch_ring_class<k_ring_subdft<MODE, WSYM>>(pl, c, nb, io);
    }
    HX_HIP(hipGetLastError());
    return HX_OK;
}

int hx::launch_ring_subdft_maps(hx_plan *pl, int nb, const double *d_maps, const double *d_pw, double2 *Y, int rp_lo, int rp_hi)
{
    ProfScope ps("ring_fft");
    if (d_pw && pl->pw_checked != d_pw) HX_TRY(classify_pixel_weights(pl, d_pw));  // (entry points that did not do it themselves)
    const RingIO io = {d_maps, d_pw, nullptr, Y, nullptr, nullptr};
    // a weight array with the symmetry of healpy's full weights goes to the WSYM kernels (see k_ring_subdft)
    return d_pw && pl->pw_mode == 2 ? launch_subdft_classes<0, true>(pl, nb, io, rp_lo, rp_hi) : launch_subdft_classes<0, false>(pl, nb, io, rp_lo, rp_hi);
}

// inverse sub-DFTs of nc components whose read-out writes the pixels (or the residual ref - synthesised of a Jacobi iteration) itself
int hx::launch_ring_subdft_spectra(hx_plan *pl, int nc, const double2 *zin, double *pixout, const double *ref)
{
    return launch_subdft_classes<1, false>(pl, nc, RingIO{nullptr, nullptr, zin, nullptr, pixout, ref});
}

// Called by the entry points of the C ABI right after they have bound their pixel-weight array, before they queue anything else:
// the host waits for a 4-byte verdict (pl->pw_mode: 1 generic, 2 symmetric), which holds for this array until the next entry.
int hx::classify_pixel_weights(hx_plan *pl, const double *d_pw)
{
    pl->pw_checked = d_pw;
    pl->pw_mode = 0;
    if (!d_pw || pl->nside < 1) return HX_OK;
    HX_TRY(pl->pw_sym.alloc(sizeof(int)));
    HX_HIP(hipMemsetAsync(pl->pw_sym.p, 1, sizeof(int), rt().stream));
    hipLaunchKernelGGL(k_pixw_symmetry, dim3(pl->nrp), dim3(256), 0, rt().stream, pl->dev(), d_pw, pl->pw_sym.as<int>());
    int flag = 0;
    HX_HIP(hipMemcpyAsync(&flag, pl->pw_sym.p, sizeof(int), hipMemcpyDeviceToHost, rt().stream));
    HX_HIP(hipStreamSynchronize(rt().stream));
    pl->pw_mode = flag != 0 ? 2 : 1;
    return HX_OK;
}
