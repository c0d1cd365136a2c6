/* hxsht.h -- C ABI of libhxsht.so, the MI355X (gfx950) harmonic-space two-point engine.
 *
 * Drop-in boundary for the hot path of heracles-ec/heracles.  The
 * reference is pure Python and binds no native library itself; each entry point below
 * replaces the third-party / numpy call the reference makes at the cited file:line, and
 * INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every pointer argument may be a HOST pointer or a
 *    DEVICE (HBM) pointer; the library detects which (hipPointerGetAttributes) and stages
 *    host buffers through its own device scratch.  The caller owns all buffers.
 *  - Complex arrays are interleaved (re, im) doubles == numpy complex128.
 *  - alm layout: m-major, mmax == lmax, idx(l,m) = m*(2*lmax+1-m)/2 + l
 *    (heracles/twopoint.py:90-99, heracles/ducc.py:157-161).
 *  - Maps are HEALPix RING ordered, npix = 12*nside^2 (heracles/healpy.py:124-142).
 *  - Return value 0 = ok, negative = error; message via hx_last_error() (thread local).
 *  - Calls are synchronous on return unless hx_set_async(1) was called.
 *  - There is NO CPU fallback: every compute entry point fails with HX_ERR_NO_DEVICE when
 *    no gfx950 device is usable.
 *  - Threading: one host thread per process drives the library (one process per GPU).  Only hx_last_error() is
 *    thread local and only the host <-> device staging is serialised internally; plans, the runtime and the profile are not
 *    thread safe.  The library does not survive fork() (HIP does not): a child must not call into it.
 */
#ifndef HXSHT_H
#define HXSHT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HX_OK 0
#define HX_ERR_ARG (-1)
#define HX_ERR_NO_DEVICE (-2)
#define HX_ERR_HIP (-3)
#define HX_ERR_MEM (-4)
#define HX_ERR_UNSUPPORTED (-5)

typedef struct hx_plan hx_plan;

/* ---- runtime ------------------------------------------------------------------- */
const char *hx_version(void);
const char *hx_last_error(void);
int hx_device_count(void);
int hx_init(int device);          /* select device, create the library stream           */
int hx_set_stream(void *stream);  /* use a caller-owned hipStream_t (NULL = own stream)  */
void *hx_get_stream(void);
int hx_set_async(int on);         /* 1: do not synchronise before returning (device ptrs) */
int hx_synchronize(void);
/* dst <- src (bytes), either side host or device memory; host <-> device through the library's pinned staging pipeline (~55 GB/s
 * from / to pageable memory).  Complete on return. */
int hx_copy(void *dst, const void *src, int64_t bytes);
/* Page-locked host memory the CALLER owns: a destination (or source) of this kind is reached by DMA directly, without the staging
 * copy and without first-touch page faults -- the buffer a caller keeps and passes again as `out` of hx_mixmat_eb / hx_mixctx_apply
 * for every matrix of a loop (the reference hands each result to its `out` mapping and drops it, heracles/twopoint.py:393-397).
 * hx_host_free(NULL) is a no-op.  The memory stays valid until freed, across hx_init calls. */
int hx_host_alloc(int64_t bytes, void **out);
int hx_host_free(void *p);

/* HIP-event timers on the library stream (bench.py's timed region / roofline). */
int hx_timer_start(void);
int hx_timer_stop(float *ms);
/* per-kernel profile: accumulate HIP-event durations of every launch of the named kernel family:
 * "ring_fft", "fourier_combine", "legendre_analysis" (all analysis kernels; also split into "legendre_analysis_s0" /
 * "legendre_analysis_s2" by spin and "legendre_valu" for the single-map vector-unit kernel), "alm_reduce", "legendre_synthesis",
 * "alm2cl", "mixmat_gemm", "wigner_tables".  hx_profile_get returns launches and total milliseconds. */
int hx_profile_enable(int on);
int hx_profile_reset(void);
int hx_profile_get(const char *name, int *launches, double *total_ms);

/* ---- spherical harmonic transforms --------------------------------------------- */
/* Replaces healpy.map2alm / alm2map as called at heracles/healpy.py:183-189 and
 * heracles/io.py:377.  A plan owns ring tables, recursion tables, Bluestein tables and
 * device scratch for up to max_comp map components per call. */
hx_plan *hx_plan_create(int nside, int lmax, int max_comp);
/* Longest ring FFT kept in LDS by plans created afterwards (power of two in [16, 8192], default 8192); Bluestein rings of up to
 * twice that run as two half-length passes.  A tuning / test knob: results do not depend on it beyond rounding. */
int hx_set_max_lds_fft(int points);
void hx_plan_destroy(hx_plan *plan);
int64_t hx_plan_scratch_bytes(const hx_plan *plan);
/* Frees the plan's transient HBM scratch (ring spectra, Legendre operands and rows, staging buffers of host maps, residual maps,
 * synthesis tables: up to ~200 GB after a full-size job).  Everything is allocated again on demand; the tables of the plan stay. */
int hx_plan_release_scratch(hx_plan *plan);
/* Lead-in table of the batched Legendre analysis (5 or more spin-0 maps / 3 or more spin-2 fields per sweep).  What a ring group
 * computes before its first matrix instruction depends on the plan only, so its chain states at that point are kept in HBM (built by
 * the kernel's own code on the first such sweep; 1.3 GB per spin at nside 4096 / lmax 6144; counted by hx_plan_scratch_bytes, freed
 * by hx_plan_release_scratch and rebuilt on the next use) and every later sweep resumes from them.  The alms are bit-identical with
 * and without.  on = 0 runs every ring group from its seeds; on = 1 (default) keeps the table of the spin-2 sweeps, which it makes
 * faster; on = 2 keeps one for the spin-0 sweeps as well (as much memory again, fewer vector instructions, no gain in time: their
 * lead-in hides under matrix work).  The table of a task set is not built -- and its sweeps run from the seeds -- if it would exceed
 * the cap (bytes; 0 = the default of 8 GiB) or a tenth of the device memory that is free once the sweep's scratch stands.  The cap
 * is applied when a table is built: lowering it does not drop a larger table that exists (hx_plan_release_scratch does). */
int hx_plan_set_leadin_resume(hx_plan *plan, int on);
int hx_plan_set_leadin_cap(hx_plan *plan, int64_t bytes);
/* HBM the analysis may use for the operands and ring-group partial sums of ONE m-chunk (bytes; a chunk always
 * holds at least one m).  0 (default) = min(80 GB, half of the free HBM); the environment variable
 * HX_SCRATCH_GB sets the initial value.  The result does not depend on the chunking (tests/test_gpu_sht.py). */
int hx_set_scratch_budget(double bytes);
/* m-chunks the most recent analysis sweep of this plan was cut into (diagnostic / tests). */
int hx_plan_last_chunks(const hx_plan *plan);
/* Measurement aid: what this device sustains, from micro-kernels repeated for ~0.25 s each (clock settled): out4 = { HBM read GB/s,
 * HBM copy GB/s (read + write), FP64 MFMA 16x16x4 TFLOP/s, FP64 VALU FMA TFLOP/s }.             */
int hx_measure_peaks(double *out4);
/* Shader clock in GHz held during the FP64 MFMA probe of the last hx_measure_peaks call (0 before any). */
double hx_measured_mfma_clock(void);
/* Shader clock in GHz held UNDER the mixing-matrix GEMM since the last call of this function (every 64th tile samples s_memtime /
 * s_memrealtime around its work); 0 when no such tile has run.  Measurement aid for bench.py's gemm_frac_of_fp64_mfma_peak. */
double hx_mixmat_gemm_clock(void);
/* Measurement aid (bench.py's roofline): matrix-instruction flops one hx_map2alm(niter = 0) of
 * ncomp components EXECUTES (task list x MFMAs per wave-block), as opposed to the algorithmic
 * 8 * 2 nside * nlm per component the roofline is quoted on.                              */
int hx_plan_mfma_flops(hx_plan *plan, int spin, int ncomp, double *flops);
/* out2[0] = the same, out2[1] = FP64 vector flops of the recursions (4 per value of lambda_lm(theta) generated). */
int hx_plan_executed_flops(hx_plan *plan, int spin, int ncomp, double *out2);
/* What the Legendre analysis kernels of this process EXECUTED since the last reset, counted by the kernels themselves (one
 * atomic per wave): out2[0] = FP64 flops of the matrix instructions issued (stages whose rings are all still dead -- below 2^-100 (spin 2) / 2^-300 (spin 0) -- issue
 * none -- the task-list figure above counts them), out2[1] = FP64 flops on the vector unit.  reset != 0 zeroes the counters.
 * bench.py's roofline.achieved is these / the kernels' HIP-event time; it agrees with the SQ_INSTS_VALU_MFMA_F64 counter. */
int hx_executed_flops(double *out2, int reset);

/* spin  : any spin weight s >= 0 (negative: HX_ERR_ARG).  0 and 2 have kernels of their own, also for batches; any other
 *         weight runs one sweep per field of the vector-unit kernels that take s at run time (analysis and synthesis, every niter),
 *         in the convention of HEALPix's map2alm_spin / alm2map_spin (rows l < s of the alms are zero / not read; s > lmax: zero alms /
 *         zero maps).  HX_SPIN_GENERIC=1 (read per call; a test hook) sends spin 2 through those sweeps as well.
 * maps  : [ncomp][npix] double; spin s >= 1: components come in (Q,U) pairs, ncomp even (odd: HX_ERR_ARG)
 * alms  : [ncomp][nlm] complex; spin s >= 1: (E,B) pairs
 * ring_weights : NULL or [2*nside] quadrature weights of ring pairs (north ring 1..2nside)
 * pix_weights  : NULL or [npix] per-pixel weights (healpy use_pixel_weights=True data).  An array that repeats over the four
 *                quadrants of every ring and from north to south -- healpy's weights do -- is recognised per call and read
 *                once per pixel pair instead of eight times; any other array is used as it is
 * fl    : NULL or [lmax+1] filter applied to the output, alm[l,m] *= fl[l]
 *         (pixel-window deconvolution, heracles/healpy.py:172-196)
 * niter : Jacobi refinement iterations (healpy's `iter`)                              */
int hx_map2alm(hx_plan *plan, int spin, int ncomp, const double *maps, double *alms,
               const double *ring_weights, const double *pix_weights, const double *fl,
               int niter);
int hx_alm2map(hx_plan *plan, int spin, int ncomp, const double *alms, double *maps);
/* The loop of heracles/mapping.py:151-172 (one transform per (field, bin) map) as ONE call over njobs transforms
 * (spins[j], ncomps[j], maps[j], alms[j], fls[j] as in hx_map2alm; fls may be NULL; niter = 0): host maps of all jobs share one
 * upload pipeline that the transforms follow slab of rings by slab of rings, so that the call costs its PCIe time plus a twelfth of one
 * sweep.  Put large jobs first.  Results are bit-identical to those of njobs hx_map2alm calls on the same (host or device) maps.
 * Spin 0 and 2 only (as hx_map2alm_list, hx_ring_modes / hx_legendre_from_modes): any other weight is HX_ERR_UNSUPPORTED here. */
int hx_map2alm_multi(hx_plan *plan, int njobs, const int *spins, const int *ncomps, const double *const *maps, double *const *alms,
                     const double *ring_weights, const double *pix_weights, const double *const *fls);
/* The same for SEPARATE arrays, as heracles holds them (heracles/mapping.py:151-172: one array per (field, bin)): map i is
 * maps[i] -- [npix] for spin 0, [2][npix] (Q, U) for spin 2 --, its alm goes to alms[i] ([nlm] / [2][nlm] complex); host or
 * device pointers.  The maps are gathered sweep by sweep into the upload pipeline of hx_map2alm_multi (no stacked host copy),
 * spin-2 fields first; fl0 / fl2: NULL or the [lmax+1] filter of the spin-0 / spin-2 maps.  niter > 0: the maps of a spin are
 * gathered into one device array first (iterations need them resident) and transformed as a batch. */
int hx_map2alm_list(hx_plan *plan, int nmaps, const int *spins, const double *const *maps, double *const *alms,
                    const double *ring_weights, const double *pix_weights, const double *fl0, const double *fl2, int niter);

/* ---- the two halves of hx_map2alm, for the m-sharded multi-GPU route (heracles/mapping.py:151-172 and
 * heracles/twopoint.py:198-215 are the loops it shards) -------------------------------------------------------------------
 * A set of orders is (first, count, step): m = first + k step, k < count; rank q of N owns (q, ., N).
 * hx_ring_modes: ring Fourier stage of ncomp maps; for every set q < nsets = (m_first[q], m_count[q], m_step) the block
 *   outs[q][comp][k][nrp_pad][4] = (F_N.re, F_N.im, F_S.re, F_S.im)(m, ring pair) with ring phase, pixel and ring weights
 *   applied (DEVICE buffers of ncomp * hx_ring_modes_size(count) doubles) -- what is sent to the rank that owns the set.
 * hx_legendre_from_modes: Legendre stage of ALL ncomp components of one spin for one set of orders: comp_modes[c] points to
 *   component c's block [count][nrp_pad][4] (as received); writes alm[c][idx(l, m)] for the orders of the set ONLY (device buffer). */
int64_t hx_ring_modes_size(const hx_plan *plan, int count);
int hx_ring_modes(hx_plan *plan, int ncomp, const double *maps, const double *pix_weights, const double *ring_weights, int nsets,
                  const int *m_first, const int *m_count, int m_step, double *const *outs);
int hx_legendre_from_modes(hx_plan *plan, int spin, int ncomp, const double *const *comp_modes, int m_first, int m_count, int m_step,
                           double *alms, const double *fl);

/* All-gather of alm shards over RCCL for hosts WITHOUT torch.distributed ("one ncclAllGather of the alm shards
 * so every rank holds all alms"; the loops being sharded are heracles/mapping.py:151-172 and heracles/twopoint.py:198-215).  In place on
 * the buffer hx_map2alm wrote: buf (device, interleaved complex) holds sum(counts) elements, rank q's shard of counts[q] complex
 * elements at offset sum_{p<q} counts[p], this rank's own shard already there; shards may differ in length (one ncclBroadcast per shard
 * in a group: over xGMI each shard travels on all links of its owner at once).  comm: an ncclComm_t the HOST created (ncclCommInitRank;
 * the library does no bootstrap); RCCL is bound at the first call (librccl.so.1), HX_ERR_UNSUPPORTED if it cannot be loaded.  The Python
 * layer does not use this: its collectives are torch.distributed's (heracles_amd/distributed.py). */
int hx_allgather_alms(void *comm, int nranks, const int64_t *counts, double *buf);

/* ---- two-point reduction -------------------------------------------------------- */
/* Replaces heracles.twopoint.alm2cl (heracles/twopoint.py:63-101) for a whole list of
 * component pairs in one launch.  alms[i] points to component i with lmax_i[i];
 * cls is [npairs][lmax_out+1]; requires lmax_out <= min over used components.         */
int hx_alm2cl_pairs(int ncomp, const int *lmax_i, const double *const *alms, int lmax_out,
                    int npairs, const int *pair_i, const int *pair_j, double *cls);
/* The same sum over the orders m0, m0 + mstep, ... < m1 only (still divided by 2l + 1): partial spectra of disjoint sets add up to
 * hx_alm2cl_pairs -- a rank's contribution on the m-sharded multi-GPU route (the loop of heracles/twopoint.py:90-99 cut by m). */
int hx_alm2cl_pairs_range(int ncomp, const int *lmax_i, const double *const *alms, int lmax_out, int npairs, const int *pair_i,
                          const int *pair_j, int m0, int m1, int mstep, double *cls);

/* ---- mixing matrices / Wigner-d ------------------------------------------------- */
/* Gauss-Legendre nodes (ascending) and weights; the `gauss_legendre` hook of
 * heracles/transforms.py:25-43. */
int hx_gauss_legendre(int n, double *x, double *w);
/* The same with every node as a double-double: node k = x[k] + xlo[k], |xlo[k]| <~ 1e-16.  The tables behind hx_mixmat / hx_mixmat_eb
 * (convolvecl.mixmat / mixmat_eb at heracles/twopoint.py:378-388) are evaluated at x + xlo: next to the poles d^l(x)' ~ l^2 / 2, and a
 * node rounded to a double shifts a matrix element at l ~ 4000 by 1e-11 of the largest
 * (tests/test_gpu_mixmat.py::test_mixmat_blocks_at_high_l_vs_3j). */
int hx_gauss_legendre_dd(int n, double *x, double *w, double *xlo);

/* Largest spin weight the Wigner-d tables and the mixing matrices serve.  The recursion in l starts from
 * d^a_{ab}(x) ~ ((1 -+ x)/2)^{(a -+ b)/2}: about (1.7e-8)^{s/2} at the polar node of an L = 6144 build, which leaves the double range
 * near s = 80; up to 32 the seed stays above 1e-125 and every error-free product of the double-double arithmetic far from the
 * denormals.  Beyond it: HX_ERR_UNSUPPORTED (not tables of zeros). */
#define HX_MAX_MIX_SPIN 32
/* D[k][l] = d^l_{ab}(x_k), l = 0..lmax, any (a,b) with max(|a|,|b|) <= HX_MAX_MIX_SPIN (zero below max(|a|,|b|), also when that
 * lies beyond lmax); out is [n][lmax+1] row-major.  (Functions of heracles/transforms.py:46-112: P_l, d20, d22, d2m2, d11, dm11, and
 * the same for every other pair.)  Test hook: env HX_WIGNER_SEED=general starts the recursion of the pairs named above from the
 * general seed as well (the results must not differ in a bit). */
int hx_wigner_d_table(int lmax, int a, int b, int n, const double *x, double *out);

/* Replaces convolvecl.mixmat / mixmat_eb as called at heracles/twopoint.py:378-388.
 * cl has ncl entries (mask spectrum, zero-extended to l3max).  out: [l1max+1][l2max+1]
 * (mixmat) or [3][l1max+1][l2max+1] (mixmat_eb: EE->EE, EE->BB, EB->EB).              */
int hx_mixmat(const double *cl, int ncl, int l1max, int l2max, int l3max, int s1, int s2,
              double *out);
int hx_mixmat_eb(const double *cl, int ncl, int l1max, int l2max, int l3max, double *out);
/* Fields of any spin weights (what heracles.twopoint.mixing_matrices hands to convolvecl for any two fields, heracles/twopoint.py:375-388),
 * spins by magnitude, up to HX_MAX_MIX_SPIN.  The matrices are DEFINED by the quadrature form
 *   G^{(ab)} = D^{(ab)T} diag(w xi) D^{(ab)} diag((2 l2 + 1)/2),  D^{(ab)}[k][l] = d^l_{ab}(x_k),
 * i.e. (-1)^{s1+s2} times the bare product of 3j symbols: a full-sky mask gives the identity for every pair of spins.
 *   hx_mixmat: (s, 0) and (0, s) for any s: G^{(s,0)}; two non-zero spins: HX_ERR_UNSUPPORTED.
 *   hx_mixmat_eb_spin: two non-zero spins, out [3][l1max+1][l2max+1] = (G^{(s1,s2)} + G^{(s1,-s2)}) / 2, (G^{(s1,s2)} - G^{(s1,-s2)}) / 2,
 *     G^{(s1,-s2)} (the roles of heracles/twopoint.py:445-458, 505-508); hx_mixmat_eb is hx_mixmat_eb_spin(2, 2). */
int hx_mixmat_eb_spin(const double *cl, int ncl, int l1max, int l2max, int l3max, int s1, int s2, double *out);
/* hx_mixmat / hx_mixmat_eb / hx_mixmat_batch keep the mask-independent part of their last build (nodes and Wigner-d tables of one
 * (l1max, l2max, l3max)) and the staging buffer of a host destination in HBM between calls (~3 GB at L = 6144), so that the next
 * build of that size allocates nothing; this frees them.  (The reference rebuilds everything per convolvecl call,
 * heracles/twopoint.py:378-388.) */
int hx_mixmat_release(void);
/* Everything the library keeps in HBM between calls OUTSIDE a plan or a context -- none of it is counted by hx_plan_scratch_bytes: the
 * cache of hx_mixmat / hx_mixmat_eb / hx_mixmat_batch (above; its staging buffer of a host destination also serves hx_mixctx_apply and
 * outlives hx_mixctx_destroy), the tables, partial sums and staging buffer hx_alm2cl_pairs keeps (<= 512 MB), and the Gauss-Legendre
 * nodes, weights and four Wigner tables hx_cl2corr / hx_corr2cl keep for their last lmax (4 (lmax + 1) ceil64(lmax + 1) doubles: 1.2 GB
 * at lmax 6144, 4.9 GB at 12288; naturalspice runs them at the mask's band limit; hx_cl2corr_cols / hx_corr2cl_cols read the same
 * tables and keep nothing of their own: index lists and factors are freed before they return).  A long-lived host
 * process of the reference's loops (heracles/twopoint.py:173-299, :316-401) calls this between stages to hand the HBM back. */
int hx_release_caches(void);
/* ---- FITS wire format of maps and alms (heracles/io.py:128-218, "next" row) ------------------------------------
 * Payload conversion between a FITS binary table of 'D' columns (row-major, big-endian) and the component-major
 * native arrays of the path, one pass on the GPU; `table` / `array` host or device.
 *   table element (row, c1, c2) <-> array[c1*s1 + c2*s2 + row*srow]
 *   maps  (io.py:128-168, ncols columns):      nc1 = ncols, nc2 = 1, s1 = nrows, srow = 1
 *   alms  (io.py:189-218, columns real, imag): nc1 = 2, nc2 = r, s1 = 1, s2 = 2*nrows, srow = 2  (complex128 (r, nrows)) */
int hx_fits_unpack_f64(int64_t nrows, int nc1, int nc2, int64_t s1, int64_t s2, int64_t srow, const void *table, double *array);
int hx_fits_pack_f64(int64_t nrows, int nc1, int nc2, int64_t s1, int64_t s2, int64_t srow, const double *array, void *table);

/* ---- catalogue tables (heracles/catalog/fits.py: the columns a FitsCatalog page holds) ---------------------------------------
 * One page of a FITS binary table -- `nrows` records of `width` (NAXIS1) bytes, big-endian, as they are in the file -- to `ncols`
 * native float64 arrays of `nrows` values, one per selected column, in one pass on the GPU.  Column c is the scalar field of TFORM
 * letter types[c] at byte offsets[c] of the record:
 *   'L' ('T' -> 1.0, any other byte -> 0.0), 'B' (unsigned byte), 'I', 'J', 'K' (signed 16 / 32 / 64 bit), 'E', 'D'.
 * Integer -> f64 and f32 -> f64 are exact; 'K' values beyond +-2^53 round to nearest even, as a C cast does.  Where tscal[c] != 1 or
 * tzero[c] != 0 the value is stored * tscal + tzero with the product rounded before the sum (no fused multiply-add): numpy's result,
 * and exact for the unsigned conventions ('I' + 32768, 'J' + 2147483648, 'B' - 128).  tscal / tzero may be NULL (no scaling).  TNULL
 * is not interpreted (fitsio does not by default either).  Fields that are not listed -- strings, vectors, descriptors -- are skipped
 * by offset.  Nothing is assumed of `width` (it may be odd) or of the alignment of `table`, a record or a field.
 * `table` (nrows * width bytes) host or device (a page-locked host table is uploaded by one asynchronous copy ahead of the kernel);
 * `columns`: ncols DEVICE pointers.  At most HX_FITS_MAX_COLUMNS columns per call.  A block stages min(1024, 48 KiB / width) records
 * (rounded down to a multiple of 64 when at least 64) in LDS; records wider than 48 KiB, and every call with HX_FITS_DIRECT in `flags`,
 * are read field by field from global memory instead (same results; the flag exists for timing and testing the two kernels). */
#define HX_FITS_MAX_COLUMNS 64
#define HX_FITS_DIRECT 1
int hx_fits_unpack_columns(int64_t nrows, int64_t width, int ncols, const int64_t *offsets, const char *types, const double *tscal,
                           const double *tzero, const void *table, double *const *columns, int flags);

/* ---- jackknife loop in HBM (heracles/dices/jackknife.py:93-248, "next" row) ------------------------------------
 * Region maps (jackknife.py:253-263: every pixel outside region k set to zero) and delete-k alms (jackknife.py:222-233,
 * :298-304: full alms minus the sum of the deleted regions' alms) without leaving the device.                      */
int hx_region_maps(int64_t npix, int ncomp, const double *maps, const double *region, double k, double *out);
int hx_alm_subtract(int64_t n, const double *full, int nsub, const double *const *subs, double *out);

/* The loop of heracles/twopoint.py:354-397 (one convolvecl call per mask pair and spin combination) as an object:
 * Gauss-Legendre nodes, Wigner-d tables and the GEMM tile list are built ONCE per (l1max, l2max, l3max); every mask streamed
 * through then costs its node weights and one GEMM per product (for jobs whose matrices do not fit in memory together).
 * kind 1: spin (0,0), 2: spin (0,2)/(2,0) -> out (l1max+1, l2max+1); 4: spin (2,2) -> out (3, l1max+1, l2max+1). */
/* The products of heracles.twopoint.apply_mixing_matrix (heracles/twopoint.py:497-524, `_M @ cl`): y[v] = M x[v] for nvec spectra
 * x [nvec][m] -> y [nvec][n], M row-major (n, m); every pointer host or device (a device-resident matrix is read once per four
 * spectra: HBM-bound).  Rows are summed in a fixed order (bitwise repeatable).                                        */
int hx_matvec(int n, int m, const double *M, int nvec, const double *x, double *y);

/* np.linalg.pinv(M, rcond) as heracles.twopoint.invert_mixing_matrix calls it (heracles/twopoint.py:447-460): out (m x n) = pseudo-inverse
 * of M (n x m, row-major), singular values <= rcond * the largest are dropped.  Blocked one-sided Jacobi SVD on the GPU (Gram matrices of
 * column-block pairs, their 64 x 64 eigenproblems in LDS, rotations), the final product on the FP64 matrix unit.  M / out host or device;
 * info (nullable, 4 doubles on the host): sweeps, singular values kept, largest, smallest kept.  Fails (HX_ERR_UNSUPPORTED, nothing
 * written to out) if the sweeps run out before the columns are orthogonal to rounding.  Unlike hx_matvec / hx_alm2cl_pairs the result
 * is NOT bitwise repeatable run to run: the Gram sums are unordered f64 atomics (differences at the 1e-16 level of the sums).       */
int hx_pinv(int n, int m, const double *M, double rcond, double *out, double *info);

typedef struct hx_mixctx hx_mixctx;
hx_mixctx *hx_mixctx_create(int l1max, int l2max, int l3max);
int hx_mixctx_apply(hx_mixctx *ctx, const double *cl, int ncl, int kind, double *out);
/* The same for any two spins (by magnitude, <= HX_MAX_MIX_SPIN): one of them zero -> one matrix (hx_mixmat), both non-zero -> three
 * (hx_mixmat_eb_spin).  kind 1 / 2 / 4 of hx_mixctx_apply are (0,0) / (2,0) / (2,2) here, bit for bit.
 * A context keeps one Wigner-d table per normalised pair (a >= |b|: (s1, s2) and (s2, s1) share theirs), built on first use:
 * (l + 1 padded to 128) x (nodes padded to 32) doubles each, 0.46 GB at L = 6144.  The (0,0) table always stays (the node weights of
 * every mask read it); of the others at most 16 (env HX_MIX_TABLES=n at hx_mixctx_create, n >= 1) are kept, enough for every pair of a
 * job with spins {0, 1, 2, 3}, and the one used longest ago is dropped for a new one. */
int hx_mixctx_apply_spin(hx_mixctx *ctx, const double *cl, int ncl, int s1, int s2, double *out);
void hx_mixctx_destroy(hx_mixctx *ctx);
/* The rows of those matrices BINNED, as heracles.twopoint.mixing_matrices(..., bins, weights) returns them (heracles/twopoint.py:391-397:
 * heracles.result.binned along axis -2, heracles/result.py:124-248 -- what heracles/cli.py:696-716 asks for whenever the configuration
 * has `bins`, e.g. `bins = 32 log 2l+1` in examples/heracles.cfg:4-6).  Binning is linear in the rows, so the numerators are formed as
 * (binned Wigner-d tables) x diag(w xi) x (tables)^T -- an (nbins x N)(N x (l2max+1)) product instead of the full matrix followed by a
 * host loop over its columns (5 s per (3, 6145, 6145) matrix in the reference's function), and only nbins x (l2max+1) doubles leave the GPU.
 *   hx_mixctx_set_bins: which [l1max+1] = bin of output multipole l (0 .. nbins-1; -1: in no bin), w [l1max+1] = its weight,
 *     norm [nbins] = the divisor of every bin (the reference: the summed weight); host arrays; the binned tables follow lazily.
 *   hx_mixctx_apply_binned: kind as hx_mixctx_apply; out (nbins, l2max+1) or (3, nbins, l2max+1), host or device;
 *     out[b][l2] = sum_{l in b} w_l M[l][l2] / norm[b], exactly 0 where the sum is exactly 0 (heracles/result.py:132-135). */
int hx_mixctx_set_bins(hx_mixctx *ctx, int nbins, const int *which, const double *w, const double *norm);
int hx_mixctx_apply_binned(hx_mixctx *ctx, const double *cl, int ncl, int kind, double *out);
int hx_mixctx_apply_binned_spin(hx_mixctx *ctx, const double *cl, int ncl, int s1, int s2, double *out); /* spins as hx_mixctx_apply_spin */
/* The same loop as ONE call over a list of masks:
 *   cls   [nmask][ncl] mask spectra; kinds [nmask] bit mask: 1 -> spin (0,0) into out00[k]; 2 -> spin (0,2)/(2,0) into
 *   out02[k]; 4 -> spin (2,2) into outeb[k] (3 matrices as hx_mixmat_eb).  Output pointers host or device. */
int hx_mixmat_batch(int nmask, const double *cls, int ncl, int l1max, int l2max, int l3max, const int *kinds,
                    double *const *out00, double *const *out02, double *const *outeb);

/* Replaces heracles.transforms._cl2corr / _corr2cl (heracles/transforms.py:115-204) for
 * nspec spectra at once: cls [nspec][lmax+1][4] <-> corrs [nspec][lmax+1][4].          */
int hx_cl2corr(int lmax, int nspec, const double *cls, double *corrs);
int hx_corr2cl(int lmax, int nspec, const double *corrs, double *cls);

/* The same transforms for batches of single COLUMNS, as FP64 GEMMs on the matrix unit against those cached tables: a column is one 1-D
 * sequence tied to one table family (0: P_l, 1: d^l_22, 2: d^l_2-2, 3: d^l_20), i.e. column 0 of hx_cl2corr with TT, column 1 with
 * EE + BB, column 2 with EE - BB, column 3 with TE; l0 = 0 for family 0 and 2 for the others.
 *   hx_cl2corr_cols: xi[c][k] = sum_{l0 <= l < nl} ((2l + 1) / 4 pi a[c][l]) T_f[l][k],        a [ncol][nl] -> xi [ncol][lmax+1]
 *   hx_corr2cl_cols: b[c][l]  = 2 pi sum_k (w_k xi[c][k]) T_f[l][k] (l0 <= l < nl), 0 (l < l0), xi [ncol][lmax+1] -> b [ncol][nl]
 * at the lmax + 1 Gauss-Legendre nodes; 1 <= nl <= lmax + 1: multipoles from nl on are not read and not written (naturalspice pads
 * data spectra to the mask's band limit and cuts them again afterwards: nl is that cut).  family [ncol] is a host array; a, xi, b host
 * or device.  A column's result is the same bits alone or at any position of any batch, and from run to run (no atomics, no split sums).
 *   hx_xi_ratio: out[c][k] = xi_d[c][k] / D^ndamp[c](alpha), alpha = xi_num[num_col[c]][k], divided by xi_den[den_col[c]][k] where
 * den_col[c] >= 0 (den_col NULL or -1: no second mask), D(alpha) = alpha (1 + exp(-k (log10 |alpha| - x0))) applied ndamp[c] times: the
 * damped mask correlation of heracles/unmixing.py:95-101 (a mask pair two data keys look up is damped twice there: ndamp = 2 for the
 * second) and the alpha of heracles/dices/jackknife.py:440-470, in plain IEEE arithmetic (alpha = 0: nan; vanishing alpha: 0 out).
 * All arrays [..][n]; num_col, den_col, ndamp [ncol] host arrays (>= 0, >= -1, >= 0); xi_* and out host or device, out may be xi_d.
 * These calls keep nothing in HBM between calls but the tables of hx_cl2corr (hx_release_caches). */
int hx_cl2corr_cols(int lmax, int nl, int ncol, const int *family, const double *a, double *xi);
int hx_corr2cl_cols(int lmax, int nl, int ncol, const int *family, const double *xi, double *b);
/* The same for columns of ANY spin weight: column c is tied to the pair pairs[c] = (a, b) (host array [ncol][2]) and runs on
 * T_{ab}[l][k] = d^l_{ab}(x_k), exactly hx_wigner_d_table(lmax, a, b) at the Gauss-Legendre nodes, with l0 = max(|a|, |b|): inputs
 * below l0 are not read, outputs below l0 are 0, l0 > lmax or l0 >= nl gives zeros.  max(|a|, |b|) > HX_MAX_MIX_SPIN: HX_ERR_UNSUPPORTED.
 * A spectrum of spins (s1, s2) is: (0,0) one column on T_00; one spin zero, the other s: a0 + a1, a0 - a1 on T_{s,0} (back (b0 +- b1)/2);
 * both non-zero: a00 + a11, a10 - a01 on T_{s1,s2} and -a01 - a10, a00 - a11 on T_{s1,-s2}.  xi of a key with odd s1 - s2 changes sign
 * with the order of the key's spins (d_{ab} = (-1)^{a-b} d_{ba}); a transform there and back does not.
 * Tables: built in double-double (the kernel of the mixing-matrix tables, nodes with their low parts), one [lmax+1][ceil64(lmax+1)]
 * table per NORMALISED pair (a >= |b|: (a,b), (b,a), (-b,-a), (-a,-b) share it, a pair that differs by the sign (-1)^{a-b} gets the
 * shared table's result negated, bit for bit), 0.31 GB each at lmax 6144.  At most HX_XI_TABLES of them are kept (env, read at first
 * use, default 8, at least 2), the one used longest ago is dropped for a new one -- also in the middle of a call whose pairs exceed
 * the bound, which changes no bit; another lmax drops all; hx_release_caches frees them.  The family entry points above do not read
 * these tables ((0,0), (2,2), (2,-2), (2,0) here agree with families 0 .. 3 to rounding, not to the bit).  Determinism as above. */
int hx_cl2corr_cols_spin(int lmax, int nl, int ncol, const int *pairs, const double *a, double *xi);
int hx_corr2cl_cols_spin(int lmax, int nl, int ncol, const int *pairs, const double *xi, double *b);
int hx_xi_ratio(int n, int ncol, const double *xi_d, const double *xi_num, const int *num_col, const double *xi_den, const int *den_col,
                const int *ndamp, double x0, double k, double *out);

/* Replaces the m-block loop of DiscreteMapper.resample (heracles/ducc.py:145-162): re-packs m-major
 * alms from band limit lmax_in to lmax_out (truncate or zero-pad).  alm_in: [ncomp][nlm(lmax_in)]
 * complex, alm_out: [ncomp][nlm(lmax_out)] complex.                                             */
int hx_alm_resample(int lmax_in, int lmax_out, int ncomp, const double *alm_in, double *alm_out);

/* ---- values at arbitrary points -> alm -----------------------------------------------------------
 * Replaces ducc0.sht.adjoint_synthesis_general(map=values, spin=spin, lmax=lmax, loc=loc, epsilon=epsilon) as called by
 * DiscreteMapper.map_values (heracles/ducc.py:121-128):  alm[c][idx(l,m)] = sum_p map[c][p] conj(sY_lm(loc[p])), m >= 0,
 * spin 0: every row of `map` on its own; spin 2: rows (Q, U) -> (E, B) with healpy's sign conventions (those of hx_map2alm).
 * Any other spin weight s >= 1 (ducc0 takes any): rows in pairs (Q, U) -> (E, B) in the convention of HEALPix's map2alm_spin,
 *   (+-s)a_lm = sum_p (Q_p +- i U_p) conj((+-s)Y_lm(loc[p])),  E = -((+s)a + (-1)^s (-s)a) / 2,  B = i ((+s)a - (-1)^s (-s)a) / 2
 * for l >= max(m, s) and zero below; s = 2 is the case above, s > lmax gives zeros.  HX_ERR_ARG: s < 0, or s > 0 with an odd ncomp.
 * loc: (npoints, 2) colatitude, longitude in radians (0 <= colatitude <= pi, else HX_ERR_ARG); map: (ncomp, npoints);
 * alm: (ncomp, nlm) complex, OVERWRITTEN (the caller adds it to its running sum, ducc.py:133); pointers host or device.
 * The object holds the non-uniform FFT of accuracy epsilon (heracles: 1e-12 for float64 values, 1e-5 for float32,
 * ducc.py:107-114) and the Legendre plan on equidistant rings; lmax <= 8191.  info4 = {lmax, N, n1, W}: rings on the
 * full circle, oversampled grid points per dimension, kernel width in cells.                                           */
typedef struct hx_pointsht hx_pointsht;
hx_pointsht *hx_pointsht_create(int lmax, double epsilon);
void hx_pointsht_destroy(hx_pointsht *ps);
int hx_pointsht_info(const hx_pointsht *ps, int *info4);
int hx_pointsht_adjoint(hx_pointsht *ps, int spin, int ncomp, int64_t npoints, const double *loc, const double *map, double *alm);
/* The forward direction, ducc0.sht.synthesis_general: map[c][p] = the field with coefficients alm at the point loc[p], for the same
 * object, spins, component rules and error codes as hx_pointsht_adjoint (HX_ERR_ARG for spin < 0, an odd ncomp with spin >= 1 and for
 * points with colatitude outside [0, pi] or non-finite coordinates, whose values are NaN).  alm: [ncomp][nlm] complex, m-major;
 * map: [ncomp][npoints] float64; host or device; npoints == 0 is valid.  s >= 1: (E, B) pairs in, (Q, U) out; s > lmax gives zeros.
 * Nothing is accumulated with atomics in this direction: a call's result is bit-identical from run to run.
 * hx_pointsht_synthesis works through the one grid the object owns, component by component.  hx_pointsht_grids does the part that
 * does not depend on the points once and keeps its result, ncomp grids of n1^2 float64 (NULL and hx_last_error when they do not fit
 * or an argument is bad); hx_pointgrid_gather then reads all components at one set of points (map: [ncomp][npoints]) and can be
 * called for page after page of a catalogue.  The hx_pointsht is BORROWED by the hx_pointgrid and has to outlive it.             */
int hx_pointsht_synthesis(hx_pointsht *ps, int spin, int ncomp, int64_t npoints, const double *loc, const double *alm, double *map);
typedef struct hx_pointgrid hx_pointgrid;
hx_pointgrid *hx_pointsht_grids(hx_pointsht *ps, int spin, int ncomp, const double *alm);
int hx_pointgrid_gather(hx_pointgrid *g, int64_t npoints, const double *loc, double *map);
void hx_pointgrid_destroy(hx_pointgrid *g);

/* ---- catalogue -> map accumulation (first "next" row of SURVEY.md 8f) ---------------
 * hx_ang2pix_ring replaces hp.ang2pix(nside, lon, lat, lonlat=True) at
 * heracles/healpy.py:157 (RING scheme, lon/lat in degrees, n points).
 * hx_map_values replaces HealpixMapper.map_values (heracles/healpy.py:144-160) with the
 * compiled loop _map (heracles/healpy.py:58-66): maps[v][ipix[j]] += values[v][j] for
 * j = 0..n-1 IN THAT ORDER per pixel (bit-identical sums; flags = 0).  values: [nval][n],
 * maps: [nval][12 nside^2], read-modify-write, host or device.  HX_MAP_ATOMIC gives up the
 * ordering guarantee for one pass of hardware f64 atomics.                             */
#define HX_MAP_ATOMIC 1
int hx_ang2pix_ring(int nside, int64_t n, const double *lon, const double *lat, int64_t *ipix);
int hx_map_values(int nside, int64_t n, const double *lon, const double *lat, int nval,
                  const double *values, double *maps, int flags);

/* Replaces hp.ud_grade(data, nside, dtype=float64) of HealpixMapper.resample
 * (heracles/healpy.py:205-209): RING in, RING out, pess=False, power=None -- degrade = mean of
 * the unmasked children (UNSEEN if none), summed in numpy's order over the NEST children
 * (pairwise within pieces of 8192, the pieces in sequence); upgrade = replication.  in: [nmaps][12 nside_in^2], out: [nmaps][12 nside_out^2].
 * Both nside must be powers of two (healpy raises ValueError otherwise; here HX_ERR_ARG).   */
int hx_ud_grade(int nside_in, int nside_out, int nmaps, const double *in, double *out);

/* NESTED <-> RING reordering of full-sky maps: what hp.read_map does to a NESTED file before heracles.io.read_vmap sees it
 * (heracles/io.py:360-365).  to_ring != 0: in is NESTED, out RING; 0: the reverse.  in / out [nmaps][12 nside^2], host or device,
 * not in place.  nside a power of two.                                                                              */
int hx_reorder(int nside, int to_ring, int nmaps, const double *in, double *out);

/* ---- catalogues -> field maps: heracles.map_catalogs with the fields of heracles/fields.py:197-559 -----------------
 * One context maps the pages of ONE catalogue into the maps of up to HX_CAT_MAX_FIELDS fields at once.  desc holds 7 ints per field:
 * {kind, nside, lon, lat, value (real part), imag, weight}, the last five indices into the column list every page passes (-1 = none;
 * a field without a weight column uses w = 1).  maps[f]: the field's DEVICE map, zeroed by the caller, [nrow][12 nside^2] with
 * nrow = 2 for HX_CAT_COMPLEX, else 1.  Fields that share (nside, lon, lat) share one ang2pix and one stable pixel sort per page.
 *  kinds:  POSITIONS adds w and keeps every row; SCALAR adds w v, COMPLEX w re and w im, WEIGHTS w, and these three drop the rows with
 *          w == 0 before anything else (their values and positions are neither checked nor added).  Products round one by one (no FMA).
 *  hx_catmap_page:    adds one page of n <= page_size rows; cols: the page's columns, host or device.  Host columns are uploaded on the
 *                     library's copy stream into one of two staging sets, so the upload of the next page overlaps this page's kernels;
 *                     the call returns once the host columns have been read (device columns: once the page is mapped).  Per pixel the
 *                     rows add in catalogue order: bit-identical to the reference's _map loop (heracles/healpy.py:58-66).
 *  hx_catmap_moments: waits for the pages, then out[4 f + k] = {n, sum w, sum w^2, sum |w v|^2} of the rows field f kept (summed per
 *                     block, then over blocks in a fixed order: bitwise repeatable) and bad[6 f + k] = the kept rows with a NaN in
 *                     {lon, lat, value, imag, weight} (k < 5) and those with an invalid position (k = 5: latitude outside [-90, 90] or a
 *                     non-finite coordinate; such rows are never added).  The caller raises on either count; the maps are then void.
 *  hx_catmap_finish:  map <- map / norm - vis (each operation rounded on its own; vis NULL: map / norm), in place.  vis: [12 nside^2],
 *                     host or device.                                                                                             */
typedef struct hx_catmap hx_catmap;
#define HX_CAT_POSITIONS 0
#define HX_CAT_SCALAR 1
#define HX_CAT_COMPLEX 2
#define HX_CAT_WEIGHTS 3
#define HX_CAT_MAX_FIELDS 8
#define HX_CAT_MAX_GROUPS 4
#define HX_CAT_MAX_COLUMNS 16
hx_catmap *hx_catmap_create(int64_t page_size, int ncols, int nfields, const int *desc, double *const *maps);
int hx_catmap_page(hx_catmap *ctx, int64_t n, const double *const *cols);
int hx_catmap_moments(hx_catmap *ctx, double *out, int64_t *bad);
int hx_catmap_finish(hx_catmap *ctx, int field, double norm, const double *vis);
void hx_catmap_destroy(hx_catmap *ctx);

/* ---- catalogues -> alms through the point transform: heracles.map_catalogs with a DiscreteMapper (heracles/ducc.py:92-133) ----------
 * hx_catmap's field kinds, rules, moments and page protocol, with the oversampled (theta, phi) grids of hx_pointsht as the accumulators:
 * the context owns one zeroed [n1][n1] float64 grid per component (2 for HX_CAT_COMPLEX, else 1; 8 n1^2 bytes each: 2.1 GB up to
 * lmax 4095, 8.6 GB for lmax 4096..8191) and every page is spread into them without clearing, so the FFT stages and the Legendre
 * analysis run once per field, in hx_catalm_finish, not once per page.  desc: 7 ints per field {kind, lmax, lon, lat, value, imag,
 * weight}; ps[f]: the point transform of field f's lmax, BORROWED (tables, sort buffers, FFT scratch, equiangular plan) and to outlive
 * the context.  Fields that share (lmax, lon, lat) share the points (theta, phi) = (radians(90 - lat), radians(lon mod 360)) and at most
 * one tile sort per page (from 300000 rows; HX_NUFFT_TILES = 0 / 1 forces the choice), then one spread per component.
 *  hx_catalm_page:    hx_catmap_page's protocol.  Rows that add nothing (kept by no field of the group, or a zero value) cost no atomics.
 *  hx_catalm_moments: as hx_catmap_moments, the same sums in the same order (bitwise repeatable); bad[6 f + 5] counts the kept rows with a
 *                     latitude outside [-90, 90] or a non-finite coordinate, which are never added.
 *  hx_catalm_finish:  alm <- (grids of the field -> alm with the given spin: 0, or any s >= 1 for a two-component field: (E, B) as
 *                     hx_pointsht_adjoint defines them; HX_ERR_ARG for s < 0 and for s > 0 on a one-component field) / norm - vis_alm,
 *                     each operation rounded on its own (vis_alm NULL: the division only).  alm: [nrow][nlm] complex, OVERWRITTEN; vis_alm:
 *                     [nlm] complex; host or device.  The grids are left as they were: a field can be finished again.
 * The spread adds with hardware float64 atomics, so the alms are NOT bit-repeatable from run to run (they agree to rounding).            */
typedef struct hx_catalm hx_catalm;
hx_catalm *hx_catalm_create(int64_t page_size, int ncols, int nfields, const int *desc, hx_pointsht *const *ps);
int hx_catalm_page(hx_catalm *ctx, int64_t n, const double *const *cols);
int hx_catalm_moments(hx_catalm *ctx, double *out, int64_t *bad);
int hx_catalm_finish(hx_catalm *ctx, int field, int spin, double norm, const double *vis_alm, double *alm);
void hx_catalm_destroy(hx_catalm *ctx);

/* ---- selections: the views of ONE base catalogue (base.where(selection)) mapped in one pass over the base's pages ------------------
 * hx_catmap_create_sel: nsel <= HX_CAT_MAX_SELECTIONS selections, the fields desc of hx_catmap_create (the same fields for every
 * selection), maps[s nfields + f] the DEVICE map of field f for selection s.  Bit s of a row's membership word is set when the base's
 * filters keep the row, its mask word has bit s (hx_catmap_page_sel) and every predicate term of selection s holds:
 *  preds:   npred <= HX_CAT_MAX_PREDICATES terms of 3 ints {selection, column, op} (op one of HX_CAT_EQ .. HX_CAT_GE), pval[npred] their
 *           constants: `column op pval` compared in float64 as numpy does (NaN: false, except HX_CAT_NE: true).
 *  filters: nfilt <= HX_CAT_MAX_FILTERS descriptors of 4 ints {type, a, b, nside}, applied in order to the rows of any selection:
 *           HX_CAT_FILTER_INVALID   a = bitmask of the columns checked, b = the weight column or -1: the row goes when one of the columns
 *                                   is NaN and (b < 0 or its weight != 0)  (heracles/catalog/filters.py:47-59);
 *           HX_CAT_FILTER_FOOTPRINT a, b = lon, lat columns; footprints[k]: the filter's DEVICE map [12 nside^2] (RING): the row goes when
 *                                   footprint[ang2pix(nside, lon, lat)] == 0; an invalid position is counted and the row goes.
 *  hx_catmap_page_sel:    hx_catmap_page plus mask[n] (host, device, or NULL: every bit set).  One stable sort per (nside, lon, lat)
 *                         group by the key (selection, pixel) serves every selection; a row in k > 1 selections enters it k times, in
 *                         catalogue order.  Per pixel every selection's rows add in catalogue order: a selection's map equals the map
 *                         of a catalogue holding exactly its rows, bit for bit.
 *  hx_catmap_moments_sel: out[4 (s nfields + f) + k] and bad[6 (s nfields + f) + k] as hx_catmap_moments, over the rows of selection s;
 *                         fcount[(nfilt + 1) s + k]: rows of s removed by filter k (k < nfilt; after the filters before it), and at
 *                         k = nfilt the rows of s with an invalid position in a footprint filter.  The moments are summed per wave and
 *                         block in a fixed order, then over blocks: bitwise repeatable (not the summation order of hx_catmap).
 *  hx_catmap_finish_sel:  hx_catmap_finish for the map of (sel, field).                                                            */
typedef struct hx_catmap_sel hx_catmap_sel;
#define HX_CAT_MAX_SELECTIONS 32
#define HX_CAT_MAX_PREDICATES 64
#define HX_CAT_MAX_FILTERS 4
#define HX_CAT_EQ 0
#define HX_CAT_NE 1
#define HX_CAT_LT 2
#define HX_CAT_LE 3
#define HX_CAT_GT 4
#define HX_CAT_GE 5
#define HX_CAT_FILTER_INVALID 0
#define HX_CAT_FILTER_FOOTPRINT 1
hx_catmap_sel *hx_catmap_create_sel(int64_t page_size, int ncols, int nfields, const int *desc, int nsel, int npred, const int *preds,
                                    const double *pval, int nfilt, const int *filters, const double *const *footprints, double *const *maps);
int hx_catmap_page_sel(hx_catmap_sel *ctx, int64_t n, const double *const *cols, const uint32_t *mask);
int hx_catmap_moments_sel(hx_catmap_sel *ctx, double *out, int64_t *bad, int64_t *fcount);
int hx_catmap_finish_sel(hx_catmap_sel *ctx, int sel, int field, double norm, const double *vis);
void hx_catmap_destroy_sel(hx_catmap_sel *ctx);

/* healpy's pixel-weight files (`healpix_full_weights_nside_NNNN.fits`, the data hp.map2alm(use_pixel_weights=True, datapath=...)
 * of heracles/healpy.py:183-189 reads): expansion of the compressed half-quadrant weights -- hx_pixel_weights_size(nside) =
 * (nside + 1)(3 nside + 1) / 4 values -- to the full-sky array [12 nside^2] of multiplicative pixel weights 1 + w that hx_map2alm
 * takes as `pix_weights`.  compressed / weights host or device.                                                           */
int64_t hx_pixel_weights_size(int nside);
int hx_pixel_weights_expand(int nside, int64_t ncompressed, const double *compressed, double *weights);
/* The compressed weights themselves, computed in HBM: the minimum-norm x with map2alm_{unit weights, band limit 2 lmax}(1 + E x) =
 * sqrt(4 pi) e_00 (E: the expansion above without the `1 +`), i.e. the weights with which map2alm(alm2map(a), niter = 0) = a for a
 * band limit lmax.  Conjugate gradients on the normal equations from x = 0, restricted to the modes the symmetries of the
 * pixelisation leave (real parts, L even, M = 0 mod 4); the host reads one scalar per iteration.  Bit-identical from run to run.
 * plan    : the HEALPix plan of (nside, 2 lmax) -- anything else is HX_ERR_ARG
 * lmax    : band limit of the transforms the weights are for, <= 3 nside / 2 (beyond that the weights make the quadrature worse:
 *           HX_ERR_ARG)
 * epsilon : stop when |gradient| <= epsilon |gradient at x = 0|; itmax: or after this many iterations (not an error)
 * compressed_out : hx_pixel_weights_size(nside) doubles, host or device
 * iterations, rel_gradient, max_residual : NULL, or the iterations used, |gradient| / |gradient at x = 0| reached, and the largest
 *           |sqrt(4 pi) e_00 - map2alm(1 + E x)| over the constrained modes, formed anew from the x handed out             */
int hx_pixel_weights_solve(hx_plan *plan, int lmax, double epsilon, int itmax, double *compressed_out, int *iterations,
                           double *rel_gradient, double *max_residual);

/* ---- HEALPix pixel window of any spin weight, computed from the pixel shapes (what healpy.pixwin reads from its data files) -----------
 * A_lm(p) = the average of sY_lm over pixel p in the local (theta, phi) basis;
 *     W_l^2 = 4 pi / ((2l+1) 12 nside^2) sum_p sum_{m=-l..l} |A_lm(p)|^2 for l >= spin, W_l = 1 for l < spin.
 * Spin 0: the definition of the HEALPix primer (W_0 = 1).  Spin s != 0: the total-power window of the pixel-averaged field, one array
 * for E and B (the E/B mixing of pixel averaging is not modelled).  Exact up to a 12-node Gauss-Legendre rule per half pixel in the
 * one coordinate the integral does not close in; bit-identical from run to run.
 * nside : 1 .. 8192, any integer;  spin : 0 .. lmax;  lmax : <= 4 nside (the rule is validated up to there) -- else HX_ERR_ARG
 * hx_pixel_window       : window [lmax + 1], host or device
 * hx_pixel_window_rings : for the northern rings ring_first .. ring_first + ring_count - 1 (1 = next to the pole, 2 nside = the equator)
 *                         the ring's own sum (4 pi / (2l+1)) sum_{p in ring} sum_m |A_lm(p)|^2 (0 for l < spin): out [ring_count][lmax + 1],
 *                         host or device.  The window is sqrt(sum_r c_r row_r / (12 nside^2)), added in ring order with c_r = 2 (the
 *                         southern twin), 1 for the equator: hx_pixel_window forms exactly this sum.                                */
int hx_pixel_window(int nside, int spin, int lmax, double *window);
int hx_pixel_window_rings(int nside, int spin, int lmax, int ring_first, int ring_count, double *out);

/* ---- covariance estimators of DICES (heracles/dices/jackknife.py:449-593, heracles/dices/shrinkage.py:66-98) ---------------------
 * Samples are stacked one per row in data-vector order; every array is row-major, host or device.  Columns are centred in two
 * passes, then every product runs on the FP64 matrix unit with K = the sample count; reductions in a fixed order (bitwise repeatable).
 *  hx_cov_gram:        out (n1 x n2) = alpha Dx^T Dy, Dx / Dy the centred columns of x (n x n1) / y (n x n2); y NULL: y = x (n2 is
 *                      ignored, only tiles I <= J are computed and mirrored).  sample_covariance (jackknife.py:504-528) is alpha =
 *                      1 / (n - 1); jackknife_covariance (:449-501) scales it by (njk - 1)^2 / njk (nd = 1) or the delete-2 factor.
 *  hx_cov_delete2:     the ensemble of delete2_correction (jackknife.py:542-552), Q[k] = njk c0 - (njk - 1) (c1[pairs[2k]] +
 *                      c1[pairs[2k + 1]]) + (njk - 2) c2[k] for c0 (N), c1 (njk x N), c2 (m x N); its columns reordered by perm
 *                      (column p of the product = data column perm[p]; NULL: identity), centred, and the Grams alpha D_b^T D_b of the
 *                      nb column slabs [bstart[b], bstart[b + 1]) written back to back into out (sum of the squared widths).
 *  hx_cov_shrink_sums: out[0] / out[1] = numerator / denominator of the optimal shrinkage factor (shrinkage.py:66-98) of the samples
 *                      x (n x N) against the target (N x N, leading dimension ldt); the W ensemble is never formed. */
int hx_cov_gram(int n, int n1, int n2, const double *x, const double *y, double alpha, double *out);
int hx_cov_delete2(int njk, int m, int N, const double *c0, const double *c1, const double *c2, const int *pairs, const int *perm,
                   int nb, const int *bstart, double alpha, double *out);
int hx_cov_shrink_sums(int n, int N, const double *x, const double *target, int64_t ldt, double *out);

/* ---- Gaussian mock alms of a set of spectra ------------------------------------------------------------------------
 * cl   : (ncomp (ncomp + 1) / 2, lmax + 1), the symmetric matrix of spectra C^{ij}_l, rows in the order of
 *        itertools.combinations_with_replacement(range(ncomp), 2) -- the array hx_alm2cl_pairs returns for that pair list
 * alms : (ncomp, nlm) complex128, a^i_lm = sum_{j <= i} L_ij(l) z^j_lm: L_l the lower Cholesky factor of C_l (no pivoting; a pivot
 *        d <= 4 ncomp 2^-52 C_jj zeroes its column), z complex standard normals from Philox4x32-10 with key (seed & 0xffffffff,
 *        seed >> 32) and counter (l, m, j, realisation): a realisation does not depend on lmax
 * chol : the factor alone, (ncomp (ncomp + 1) / 2, lmax + 1), same packing, L_ij with i >= j at the row of pair (j, i)
 * Host or device pointers, as everywhere in this header.  1 <= ncomp <= 64, lmax >= 0, else HX_ERR_ARG.  A matrix that is not positive
 * semi-definite (a pivot below -4 ncomp 2^-52 C_jj), NaN or Inf: HX_ERR_ARG, hx_last_error names the smallest such l, nothing is written.
 * The factor of the last call stays in HBM (ncomp (ncomp + 1) / 2 x (lmax + 1) doubles) until hx_release_caches. */
int hx_synalm(int ncomp, int lmax, const double *cl, uint64_t seed, uint32_t realisation, double *alms);
int hx_cl_cholesky(int ncomp, int lmax, const double *cl, double *chol);

/* ---- Lognormal mocks: Gaussianised spectra, repair of indefinite spectra, the map pass ---------------------------------
 * hx_lognormal_xi: element-wise over correlation-function columns xi [ncol][nnodes], one factor per column (factor: host array [ncol]):
 *   direction 0: out = log1p(xi * factor[c])   (to the Gaussian field: factor = 1 / (shift_i shift_j))
 *   direction 1: out = factor[c] * expm1(xi)   (to the lognormal field: factor = shift_i shift_j)
 *   in plain IEEE arithmetic, every operation rounded on its own.  out may be xi itself; any other overlap is HX_ERR_ARG.  Direction 0
 *   with an argument of log1p that is <= -1 or NaN: HX_ERR_ARG, hx_last_error names the smallest (column, node), nothing is written.
 *   Profile name "lognormal_xi".
 * hx_lognormal_maps: out[r][p] = shift[r] * expm1(g[r][p] - sigma2[r] / 2) for nrow rows (1 .. 65535) of npix >= 1 doubles; sigma2 and
 *   shift are host arrays [nrow] (shift > 0, sigma2 >= 0, finite).  out may be g itself; any other overlap is HX_ERR_ARG and nothing is
 *   written.  One streaming pass.  Profile name "lognormal_maps".
 * hx_cl_nearest_psd: cl and out packed as for hx_synalm, 1 <= ncomp <= 64.  Per l, with D = diag(C_l) and the components of C_jj = 0
 *   left out (their rows and columns come back zero): R = D^-1/2 C D^-1/2 = V L V^T by cyclic Jacobi (round-robin order, until the largest
 *   |off-diagonal| is <= 2^-50), C' = D^1/2 V max(L, floor) V^T D^1/2.  A matrix with no eigenvalue below floor is copied through bit for
 *   bit.  floor < 0 selects the default 64 ncomp^2 2^-52, with which C' passes hx_cl_cholesky without a zeroed column; 0 <= floor < 1
 *   otherwise.  change (may be NULL): [lmax + 1], max_ij |C'_ij - C_ij| / sqrt(C_ii C_jj), 0 where copied, +Inf where a non-zero entry
 *   beside a zero auto-spectrum was removed.  out may be cl itself.  A negative auto-spectrum, NaN or Inf anywhere: HX_ERR_ARG,
 *   hx_last_error names the smallest such l and the component; sweeps that do not converge: HX_ERR_UNSUPPORTED; nothing is written in
 *   either case.  The same bits in every run and for every split of the l range.  The result and the change report of the last call
 *   stay in HBM until hx_release_caches.  Profile name "cl_nearest_psd". */
int hx_lognormal_xi(int direction, int ncol, int nnodes, const double *factor, const double *xi, double *out);
int hx_lognormal_maps(int nrow, int64_t npix, const double *sigma2, const double *shift, const double *g, double *out);
int hx_cl_nearest_psd(int ncomp, int lmax, const double *cl, double floor, double *out, double *change);

/* ---- Poisson-sampled mock catalogues from expected-count maps ------------------------------------------------------
 * Both calls work on a range [pix_begin, pix_end) of RING pixels of `nside` (1 .. 8192, any integer); every array covers that range
 * only, so a catalogue can be made in pieces.  A realisation is a function of (seed, realisation, nside, pixel, index) alone.
 * hx_mockcat_counts: counts[p - pix_begin] ~ Poisson(lam[p - pix_begin]) (int64), *total (host) their sum.  A lam that is NaN,
 *   negative, infinite or above 2^30 (hx_last_error names the first such pixel), or a total >= 2^31: HX_ERR_ARG, nothing is written.
 * hx_mockcat_points: the points of those counts, sorted by pixel, then by index within the pixel: lon / lat in degrees (lon in
 *   [0, 360), the conventions of hx_ang2pix_ring), values [nval][total] with values[j][g] = maps[j][p - pix_begin] + sigma[j] x a
 *   standard normal (sigma[j] == 0 adds nothing), and, unless NULL, pix[g] = the RING pixel p of point g.  maps: [nval][pix_end -
 *   pix_begin]; total is the sum of the counts, < 2^31.  A negative count or a larger total: HX_ERR_ARG, nothing is written.
 * Host or device pointers, as everywhere in this header. */
int hx_mockcat_counts(int nside, int64_t pix_begin, int64_t pix_end, const double *lam, uint64_t seed, uint32_t realisation, int64_t *counts,
                      int64_t *total);
int hx_mockcat_points(int nside, int64_t pix_begin, int64_t pix_end, const int64_t *counts, uint64_t seed, uint32_t realisation, int nval,
                      const double *maps, const double *sigma, double *lon, double *lat, double *values, int64_t *pix);

/* ---- jackknife regions: equal-weight segmentation of a weighted footprint -------------------------------------------
 * No counterpart in the reference: its tutorial takes the region map from a third-party host package.  weight [12 nside^2] (RING,
 * nside 1 .. 8192, any integer) is cut into njk (1 .. 4096) compact regions of equal summed weight by recursive weighted bisection
 * along the principal axis: labels[p] = 0 where weight[p] <= 0, else the region 1 .. njk of pixel p.  The result is a function of
 * (nside, weight, njk) alone and bit-identical from run to run.
 * region_weight (NULL or [njk]): region_weight[k - 1] = the summed weight of label k.  axes (NULL or [(njk - 1) * 3]): axes[3 (b - 2) ..]
 * is the unit axis of the split whose right part starts at label b (every b in 2 .. njk occurs once).
 * HX_ERR_ARG, nothing written: a NaN, negative or infinite weight (hx_last_error names the first such pixel), fewer footprint pixels
 * than njk, njk or nside out of range.  Host or device pointers, as everywhere in this header. */
int hx_jk_regions(int nside, const double *weight, int njk, int32_t *labels, double *region_weight, double *axes);

/* ---- rotation of alms by any Euler angles ---------------------------------------------------------------------------
 * R = Rz(phi) Ry(theta) Rz(psi) on column vectors (psi about z first, then theta about y, then phi about z; counter-clockwise about
 * the fixed axes), rotated field f'(n) = f(R^-1 n):
 *   alm_out[c][l, m] = sum_{m' = -l .. l} exp(-i m phi) d^l_{mm'}(theta) exp(-i m' psi) alm_in[c][l, m'],
 * d^l(theta) = exp(-i theta J_y) in the Condon-Shortley basis (d^1_10 = -sin(theta) / sqrt(2)), a_l,-m' = (-1)^m' conj(a_lm'); the
 * imaginary part of a_l0 is not read and comes back as exactly 0.  alm_in, alm_out: (ncomp, nlm) complex128 in the layout of every alm
 * here (m-major, mmax = lmax); every component is rotated with the same matrices (E and B of a field of any spin weight rotate as
 * scalars).  Any finite angles: theta is brought into [0, pi] on the host ((psi, theta, phi) -> (psi - pi, -theta, phi + pi)),
 * theta = 0 and theta = pi take their closed forms; below sin(theta) = 0.1 the rotation is done as two, by pi/2 and theta - pi/2,
 * through a scratch alm of the size of the input (the FP64 recurrence loses 1 / sin(theta): DESIGN.md 4.18), at twice the time.
 * 1e-12 of max |a| holds for every angle up to lmax 6144 at least.  The sum over m' has a fixed order: the result is bit-identical from call to call
 * and does not depend on how the components are batched.
 * Host or device pointers, as everywhere in this header.  The two arrays must not overlap (every output order needs every input
 * order): HX_ERR_ARG, as are lmax < 0, ncomp < 1 and an angle that is NaN or Inf; lmax > 32000 is HX_ERR_UNSUPPORTED.  Runs on the
 * library stream; its flops are added to the vector-unit figure of hx_executed_flops; profile name "rotate_alm". */
int hx_rotate_alm(int lmax, int ncomp, const double _Complex *alm_in, double _Complex *alm_out, double psi, double theta, double phi);

/* ---- mask-aware Gaussian covariance of pseudo-Cl, narrow-kernel approximation ---------------------------------------
 * One coupling table and a list of spectra into blocks of the covariance of the (binned) data vector.  With Xi_{ll'} = g00[l][l'] /
 * (2l' + 1) and Sbar^s_{ll'} = (spec[s][l] + spec[s][l']) / 2, every item adds its block
 *   cov[(row + b) ldc + col + b'] += sum_{l in b, l' in b'} w_l w_l' Xi_{ll'} (Sbar^{s0} Sbar^{s1} + Sbar^{s2} Sbar^{s3}) / (norm_b norm_b')
 * and the call touches no other element.  s[2] < 0: the first product only.
 *   g00   : (lmax + 1)^2, the (0,0) matrix as hx_mixctx_apply (kind 1) writes it for the cross-spectrum of two mask products; the call
 *           divides the column factor out itself.  Xi is taken as symmetric (it is, to rounding, for l1max = l2max).
 *   spec  : [nspec][lmax + 1].
 *   which, w, norm : the bins of both axes as in hx_mixctx_set_bins, HOST arrays; an empty bin adds nothing.  nbins = 0: every l is
 *           its own bin with weight 1 (blocks of edge lmax + 1), formed element by element.
 *   items : HOST array; the blocks of one call must not overlap (HX_ERR_ARG: each element has one owner; use two calls).
 *   cov   : DEVICE memory, leading dimension ldc.  g00 and spec host or device.
 * Binned calls fold the table once per call into Z[s][b'][l] = sum_{l' in b'} w_l' Xi_{ll'} S^s_l' for the spectra the items name and
 * the all-ones spectrum, then form each element from those rows: L^2 nspec + nitem nbins L operations instead of nitem L^2.  Z
 * ((named spectra + 1) x nbins x (lmax + 1) doubles) stays in HBM until hx_release_caches; HX_ERR_MEM, nothing written, if it does not
 * fit in 0.9 of the free memory.  No floating-point atomics: a block has the same bits in every run and whatever other items share
 * the call.  HX_ERR_ARG, nothing written: a null pointer, a spectrum index outside [0, nspec), a block that leaves ldc, a negative
 * row or col, which[l] outside [-1, nbins), a zero or non-finite norm of a bin with members.  Runs on the library stream; its flops
 * (counted from the launch shapes) are added to the vector-unit figure of hx_executed_flops; profile name "gauss_cov". */
typedef struct { int64_t row, col; int s[4]; } hx_cov_item;
int hx_gauss_cov_accumulate(int lmax, const double *g00, int nspec, const double *spec, int nbins, const int *which, const double *w,
                            const double *norm, int64_t nitem, const hx_cov_item *items, double *cov, int64_t ldc);

/* ---- mask tools: disc holes, distance to the nearest masked pixel, C1 / C2 apodisation ------------------------------
 * Maps are RING, float64, nside 1 .. 8192 (any integer).  The centre v_p of pixel p is the pixel centre of the HEALPix paper; between
 * unit vectors h(u, v) = ((u_x - v_x)^2 + (u_y - v_y)^2 + (u_z - v_z)^2) / 2 = 1 - cos(angle), for an angle h(a) = 2 sin^2(a / 2); a
 * pixel is masked when mask[p] <= 0.  All angles in degrees.  A NaN or infinite mask value (hx_last_error names the first such
 * pixel), nside out of range, a null pointer: HX_ERR_ARG, nothing is written.  Host or device pointers, as everywhere in this header.
 * hx_mask_discs: mask[p] = 0.0 wherever h(v_p, c_k) <= h(radius_k) for some disc k, c_k = (cos lat cos lon, cos lat sin lon, sin lat):
 *   the pixel centres inside the discs (query_disc, inclusive = False).  mask is changed in place.  radius: [ndisc], or NULL for
 *   radius_all on every disc.  The result does not depend on the order of the discs and is bit-identical from run to run.  ndisc = 0
 *   writes nothing.  HX_ERR_ARG, nothing written: a NaN or infinite coordinate, |lat| > 90, a radius outside [0, 180]
 *   (hx_last_error names the first such disc).  HX_MASK_WIDE=1 (tests) sends every disc down the work-group-per-disc path.
 * hx_mask_distance: H[p] = min(h(max_distance), min over masked q of h(v_p, v_q)), 0 on masked pixels, the cap everywhere for a mask
 *   without masked pixels; the angle is 2 asin(sqrt(H / 2)).  max_distance in (0, 180].
 * hx_mask_taper: out[p] = mask[p] w(sqrt(H[p] / h(aposize))) with H capped at h(aposize), 0.0 on masked pixels; kind 1 (C1):
 *   w = x - sin(2 pi x) / (2 pi); kind 2 (C2): w = (1 - cos(pi x)) / 2 -- NaMaster's mask_apodization of those names.  aposize in
 *   (0, 180]; any other kind is HX_ERR_ARG.  out may be mask itself (any other overlap is HX_ERR_ARG).
 * Both are bit-identical from run to run (a minimum does not depend on the order).  Profile names "mask_discs", "mask_neighbours",
 * "mask_distance". */
int hx_mask_discs(int nside, double *mask, int64_t ndisc, const double *lon, const double *lat, const double *radius, double radius_all);
int hx_mask_distance(int nside, const double *mask, double max_distance, double *H);
int hx_mask_taper(int nside, const double *mask, double aposize, int kind, double *out);

/* hx_mask_polygons: mask[p] = value for every pixel whose centre lies inside at least one of npoly convex spherical
 * polygons.  Polygon k has the vertices offsets[k] .. offsets[k + 1] - 1 of lon, lat (degrees), 3 .. 64 of them, in either winding; its
 * edges are the minor great-circle arcs between consecutive vertices.  With v_k = (cos lat cos lon, cos lat sin lon, sin lat),
 * n_e = v_k x v_(k+1) (each component the difference of two products), d(u, e) = (n_x u_x + n_y u_y) + n_z u_z and sigma = +1 if
 * d(v_2, e_0) > 0, else -1, all in float64 without fused multiply-adds: pixel p is inside iff sigma d(v_p, e) >= 0 for every edge --
 * query_polygon, inclusive = False.  A polygon is valid iff sigma d(v_k, e) > 0 for every edge and every vertex that is not one of its
 * endpoints (convex; no repeated vertex, collinear triple, reflex vertex or antipodal neighbours).  Every writer stores the same
 * value: the result does not depend on the order of the polygons and is bit-identical from run to run.  value = 0.0 cuts holes; a map
 * of zeros with value = 1.0 builds the union of tiles.  npoly = 0 writes nothing.  HX_ERR_ARG, nothing written (hx_last_error names
 * the first such polygon or pixel): a NaN or infinite coordinate, |lat| > 90, a vertex count outside 3 .. 64, offsets not starting at
 * 0 or decreasing, an invalid polygon, a NaN or infinite value, a NaN or infinite mask value.  offsets: [npoly + 1], host or device,
 * as mask, lon and lat.  HX_MASK_WIDE=1 (tests) sends every polygon down the work-group-per-polygon path.  Profile name
 * "mask_polygons". */
int hx_mask_polygons(int nside, double *mask, int64_t npoly, const int64_t *offsets, const double *lon, const double *lat, double value);

/* ---- template deprojection of maps ----------------------------------------------------------------------------------
 * A field's map d (already weighted by its mask v), its templates t_1 .. t_k (unmasked), f_i = v t_i; sums over pixels also run over
 * the ncomp components (1 for spin 0, else 2).  Maps and templates are [ncomp][npix] arrays, float64; `templates`, `maps` and `out`
 * are HOST arrays of pointers to them (as hx_alm_subtract); the arrays themselves, mask [npix] (NULL: all ones), gram and alpha are
 * host or device, as everywhere in this header.
 * hx_deproject_gram: with the columns X = (v t_1 .. v t_k, d_1 .. d_m), gram = X^T X, the full symmetric n x n matrix, n = ntemp + nmap,
 *   row-major: G_ij = sum f_i f_j, r_i = sum f_i d for every map, and d^T d.  The inner axis (ncomp npix elements) is cut into slabs
 *   of max(8192, ceil(ncomp npix / ceil(2048 / tiles))) elements rounded up to a multiple of 32, tiles = T (T + 1) / 2, T = ceil(n / 64):
 *   a function of the sizes alone.  A slab is accumulated in ascending order on the FP64 matrix unit, the slabs are added in ascending
 *   order; no floating-point atomics: the same bits in every run and on every device, and gram is exactly symmetric.  HX_DEPROJ_SLAB=n
 *   (tests, read at every call) sets the slab length.  Partial tiles (tiles x slabs x 32 KiB, at most ~72 MB) and the reduced matrix
 *   stay in HBM until hx_release_caches; HX_ERR_MEM, nothing written, if they do not fit in 0.9 of the free memory.  HX_ERR_ARG, nothing
 *   written: npix < 1, ncomp outside {1, 2}, ntemp < 0, nmap < 0, n outside 1 .. 1024, a null pointer, gram overlapping an input, and a
 *   diagonal entry of the result that is not finite -- hx_last_error names the first such column, a template or a map that holds a NaN
 *   or an infinite value.  Flops are added to the matrix-unit figure of hx_executed_flops; profile name "deproject_gram".
 * hx_deproject_apply: out[m][c][p] = maps[m][c][p] - v(p) * (sum_i alpha[m][i] * templates[i][c][p]); the sum starts from 0.0 at i = 0
 *   and runs in ascending order, every product and every sum rounds on its own (the kernel is compiled with floating-point
 *   contraction off: no fused multiply-add), the product with v comes last (skipped for mask NULL), the subtraction is separate.
 *   alpha: [nmap][ntemp].  out[m] may be maps[m] itself; any other overlap of an output with an input or another output is HX_ERR_ARG,
 *   as are the argument errors above (ntemp 0 .. 1024; nmap = 0 writes nothing).  One streaming pass: a template element is read once
 *   for up to 8 maps.  Profile name "deproject_apply".
 * hx_alm_apply_cl: alm_out[x][l, m] = sum_y cl[x][y][l] alm_in[y][l, m]; cl [nout][nin][lmax + 1], alms in the layout of every alm here
 *   (m-major, mmax = lmax), nin and nout 1 or 2.  Input and output must not overlap (HX_ERR_ARG).  Profile name "alm_apply_cl". */
int hx_deproject_gram(int64_t npix, int ncomp, int ntemp, const double *const *templates, int nmap, const double *const *maps,
                      const double *mask, double *gram);
int hx_deproject_apply(int64_t npix, int ncomp, int ntemp, const double *const *templates, const double *mask, int nmap,
                       const double *const *maps, const double *alpha, double *const *out);
int hx_alm_apply_cl(int lmax, int nin, int nout, const double *cl, const double _Complex *alm_in, double _Complex *alm_out);

#ifdef __cplusplus
}
#endif
#endif
