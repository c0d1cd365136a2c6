// hx_fits.hip -- payload conversion of the FITS binary tables Heracles keeps its maps and alms in
// (heracles/io.py:128-218: maps as HEALPix RING IMPLICIT FULLSKY tables, one column per map component; alms as the two
// columns "real" / "imag").  A FITS table is ROW-major and BIG-endian: row r holds its value of every column.  The arrays
// of the path are component-major and native-endian.  The byte swap and the (de)interleave are one HBM-bound pass over the
// payload on the GPU, straight from / into the device arrays the transforms work on, instead of numpy's
// astype / moveaxis / ascontiguousarray copies on one host core.
//
//   table element (row, c1, c2), c = c1 * nc2 + c2 the position within the row  <->  array[c1 * s1 + c2 * s2 + row * srow]
//     maps (ncols columns 'D'):            nc1 = ncols, nc2 = 1,  s1 = nrows,  srow = 1
//     alms (columns real, imag 'rD'):      nc1 = 2 (re, im), nc2 = r,  s1 = 1,  s2 = 2 * nrows,  srow = 2   (complex128, shape (r, nrows))
#include "hx_common.h"

#include <algorithm>

namespace hx {
namespace {

__device__ inline unsigned long long bswap64(unsigned long long v) { return __builtin_bswap64(v); }

struct FitsLayout {
    long long nrows;
    int nc1, nc2;
    long long s1, s2, srow;
};

// lanes run along the table row (coalesced on the table side); the array side is strided by construction of the format
template <bool UNPACK>
__global__ __launch_bounds__(256) void k_fits_f64(FitsLayout L, const unsigned long long *__restrict__ src,
                                                  unsigned long long *__restrict__ dst)
{
    const long long nc = (long long)L.nc1 * L.nc2, total = L.nrows * nc;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long st = (long long)gridDim.x * blockDim.x;
    for (; i < total; i += st) {
        const long long row = i / nc;
        const int c = (int)(i - row * nc), c1 = c / L.nc2, c2 = c - c1 * L.nc2;
        const long long a = c1 * L.s1 + c2 * L.s2 + row * L.srow;
        if (UNPACK) dst[a] = bswap64(src[i]);
        else dst[i] = bswap64(src[a]);
    }
}

int fits_convert(bool unpack, int64_t nrows, int nc1, int nc2, int64_t s1, int64_t s2, int64_t srow, const void *src, void *dst)
{
    HX_TRY(ensure_ready());
    if (nrows < 0 || nc1 < 1 || nc2 < 1 || !src || !dst) return fail(HX_ERR_ARG, "hx_fits_%s_f64: bad arguments", unpack ? "unpack" : "pack");
    if (nrows == 0) return HX_OK;
    const size_t n = (size_t)nrows * nc1 * nc2;
    // extent of the array side (strides are non-negative by contract)
    if (s1 < 0 || s2 < 0 || srow < 0) return fail(HX_ERR_ARG, "hx_fits: negative stride");
    const size_t extent = (size_t)((nc1 - 1) * s1 + (nc2 - 1) * s2 + (nrows - 1) * srow + 1);
    InView vin;
    OutView vout;
    HX_TRY(vin.bind(src, sizeof(double) * (unpack ? n : extent)));
    HX_TRY(vout.bind(dst, sizeof(double) * (unpack ? extent : n)));
    FitsLayout L = {nrows, nc1, nc2, s1, s2, srow};
    ProfScope ps(unpack ? "fits_unpack" : "fits_pack");
    if (unpack)
        hipLaunchKernelGGL(k_fits_f64<true>, dim3(4096), dim3(256), 0, rt().stream, L, vin.as<unsigned long long>(), vout.as<unsigned long long>());
    else
        hipLaunchKernelGGL(k_fits_f64<false>, dim3(4096), dim3(256), 0, rt().stream, L, vin.as<unsigned long long>(), vout.as<unsigned long long>());
    HX_HIP(hipGetLastError());
    HX_TRY(vout.finish());
    HX_HIP(hipStreamSynchronize(rt().stream));
    return HX_OK;
}


// ---- catalogue tables: selected scalar columns of mixed type -> one float64 array each ------------------------------------------
// A catalogue record is NAXIS1 bytes wide -- any width, odd ones included -- and a page of records may start at any byte, so neither a
// record nor a field is aligned.  Two kernels decode it (flag HX_FITS_DIRECT selects the second; DESIGN.md section 4.9 has both times):
//   tile:   a block copies a run of whole records to LDS with 16-byte loads (head and tail bytes singly, so that nothing outside the
//           page is read), then lane = row: every field is cut from LDS and stored along rows, coalesced on both sides of HBM;
//   direct: one thread per (row, column) gathers its field from global memory byte by byte.
// Both decode through the same function, so they agree bit for bit.
struct FitsCols {
    int n;
    int off[HX_FITS_MAX_COLUMNS];
    unsigned char type[HX_FITS_MAX_COLUMNS];    // TFORM letter: L B I J K E D
    unsigned char scaled[HX_FITS_MAX_COLUMNS];  // TSCAL != 1 or TZERO != 0
    double scal[HX_FITS_MAX_COLUMNS], zero[HX_FITS_MAX_COLUMNS];
    double *out[HX_FITS_MAX_COLUMNS];
};

constexpr int FITS_TILE_LDS = 48 * 1024;  // bytes of records per tile: three blocks share the 160 KiB of a CU
constexpr int FITS_TILE_PAD = 32;         // up to 15 bytes of alignment shift in front, the over-read of lds_field behind
constexpr int FITS_TILE_MAX_ROWS = 1024;

__host__ __device__ inline int field_bytes(unsigned char t)
{
    switch (t) {
    case 'L': case 'B': return 1;
    case 'I': return 2;
    case 'J': case 'E': return 4;
    case 'K': case 'D': return 8;
    }
    return 0;
}

// rows of one tile for records of `width` bytes; 0: a record does not fit, the direct kernel reads the table
inline int tile_rows(int64_t width)
{
    if (width < 1 || width > FITS_TILE_LDS) return 0;
    int r = (int)std::min<int64_t>(FITS_TILE_MAX_ROWS, FITS_TILE_LDS / width);
    return r >= 64 ? r & ~63 : r;
}

// stored * TSCAL + TZERO as numpy computes it: the product is rounded before the sum (no fused multiply-add), which makes the unsigned
// conventions (I with TZERO 32768, J with 2147483648, B with -128) exact
__device__ inline double scale_unfused(double x, double s, double z)
{
#pragma clang fp contract(off)
    const double p = x * s;
    return p + z;
}

// v: the field's bytes as a big-endian integer, right-aligned.  Integer -> f64 and f32 -> f64 are exact; K beyond +-2^53 rounds to
// nearest even, as the C cast does.  L: 'T' is 1, every other byte 0.  TNULL is not interpreted.
__device__ inline double decode_field(unsigned long long v, unsigned char t)
{
    switch (t) {
    case 'L': return (v & 0xff) == 'T' ? 1.0 : 0.0;
    case 'B': return (double)(unsigned)(v & 0xff);
    case 'I': return (double)(short)v;
    case 'J': return (double)(int)v;
    case 'K': return (double)(long long)v;
    case 'E': return (double)__uint_as_float((unsigned)v);
    default: return __longlong_as_double((long long)v);
    }
}

// the n bytes at byte offset o of LDS as a right-aligned big-endian integer, from three aligned words (the last may lie in the pad)
__device__ inline unsigned long long lds_field(const unsigned *lds32, int o, int n)
{
    const int a = o >> 2, sh = (o & 3) * 8;
    const unsigned long long lo = lds32[a] | ((unsigned long long)lds32[a + 1] << 32);
    const unsigned long long w2 = lds32[a + 2];
    const unsigned long long v = sh ? (lo >> sh) | (w2 << (64 - sh)) : lo;
    return bswap64(v) >> (64 - 8 * n);
}

__global__ __launch_bounds__(256) void k_fits_columns_tile(FitsCols C, long long nrows, int width, int tile, const unsigned char *__restrict__ table)
{
    extern __shared__ uint4 lds_raw[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_raw);
    const int tid = threadIdx.x;
    const long long ntiles = (nrows + tile - 1) / tile;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long r0 = t * tile;
        const int nr = (int)min((long long)tile, nrows - r0), nb = nr * width;
        const unsigned char *g = table + r0 * width;
        // the records keep their position within a 16-byte word, so the wide loads and stores are both aligned
        const int shift = (int)(reinterpret_cast<uintptr_t>(g) & 15);
        const int head = min(nb, (16 - shift) & 15);
        if (tid < head) lds[shift + tid] = g[tid];
        const int nvec = (nb - head) >> 4;
        const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
        uint4 *lv = reinterpret_cast<uint4 *>(lds + shift + head);
        for (int i = tid; i < nvec; i += blockDim.x) lv[i] = gv[i];
        const int done = head + (nvec << 4);
        if (tid < nb - done) lds[shift + done + tid] = g[done + tid];
        __syncthreads();
        for (int r = tid; r < nr; r += blockDim.x)
            for (int c = 0; c < C.n; ++c) {
                const unsigned char ty = C.type[c];
                double x = decode_field(lds_field(reinterpret_cast<const unsigned *>(lds), shift + r * width + C.off[c], field_bytes(ty)), ty);
                if (C.scaled[c]) x = scale_unfused(x, C.scal[c], C.zero[c]);
                C.out[c][r0 + r] = x;
            }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_fits_columns_direct(FitsCols C, long long nrows, long long width, const unsigned char *__restrict__ table)
{
    const int c = blockIdx.y;
    const unsigned char ty = C.type[c];
    const int n = field_bytes(ty);
    const long long st = (long long)gridDim.x * blockDim.x;
    for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < nrows; row += st) {
        const unsigned char *p = table + row * width + C.off[c];
        unsigned long long v = 0;
        for (int b = 0; b < n; ++b) v = (v << 8) | p[b];
        double x = decode_field(v, ty);
        if (C.scaled[c]) x = scale_unfused(x, C.scal[c], C.zero[c]);
        C.out[c][row] = x;
    }
}

int fits_unpack_columns(int64_t nrows, int64_t width, int ncols, const int64_t *offsets, const char *types, const double *tscal,
                        const double *tzero, const void *table, double *const *out, int flags)
{
    HX_TRY(ensure_ready());
    if (nrows < 0 || width < 1 || width > INT32_MAX || ncols < 1 || !offsets || !types || !out || (nrows > 0 && !table))
        return fail(HX_ERR_ARG, "hx_fits_unpack_columns: bad arguments");
    if (ncols > HX_FITS_MAX_COLUMNS) return fail(HX_ERR_ARG, "hx_fits_unpack_columns: %d columns in one call (at most %d)", ncols, HX_FITS_MAX_COLUMNS);
    FitsCols C;
    memset(&C, 0, sizeof C);
    C.n = ncols;
    for (int c = 0; c < ncols; ++c) {
        const int n = field_bytes((unsigned char)types[c]);
        if (!n) return fail(HX_ERR_UNSUPPORTED, "hx_fits_unpack_columns: column %d has type '%c' (one of L B I J K E D)", c, types[c]);
        if (offsets[c] < 0 || offsets[c] + n > width)
            return fail(HX_ERR_ARG, "hx_fits_unpack_columns: column %d ('%c' at byte %lld) lies outside the record of %lld bytes", c, types[c],
                        (long long)offsets[c], (long long)width);
        if (nrows > 0 && !is_device_ptr(out[c])) return fail(HX_ERR_ARG, "hx_fits_unpack_columns: output %d is not device memory", c);
        C.off[c] = (int)offsets[c];
        C.type[c] = (unsigned char)types[c];
        C.scal[c] = tscal ? tscal[c] : 1.0;
        C.zero[c] = tzero ? tzero[c] : 0.0;
        C.scaled[c] = C.scal[c] != 1.0 || C.zero[c] != 0.0;
        C.out[c] = out[c];
    }
    if (nrows == 0) return HX_OK;
    InView vin;
    HX_TRY(vin.bind(table, (size_t)nrows * (size_t)width));
    const int tile = (flags & HX_FITS_DIRECT) ? 0 : tile_rows(width);
    if (tile) {
        ProfScope ps("fits_columns_tile");
        const long long ntiles = (nrows + tile - 1) / tile;
        const unsigned grid = (unsigned)std::min<long long>(ntiles, (long long)rt().cus * 8);
        const size_t lds = (((size_t)tile * (size_t)width + 15) & ~(size_t)15) + FITS_TILE_PAD;  // (what the tile holds, not the budget)
        hipLaunchKernelGGL(k_fits_columns_tile, dim3(grid), dim3(256), lds, rt().stream, C, (long long)nrows, (int)width,
                           tile, vin.as<unsigned char>());
    } else {
        ProfScope ps("fits_columns_direct");
        const unsigned grid = (unsigned)std::min<long long>((nrows + 255) / 256, 65536);
        hipLaunchKernelGGL(k_fits_columns_direct, dim3(grid, ncols), dim3(256), 0, rt().stream, C, (long long)nrows, (long long)width,
                           vin.as<unsigned char>());
    }
    HX_HIP(hipGetLastError());
    HX_HIP(hipStreamSynchronize(rt().stream));  // (the temporary of a host table is freed on return)
    return HX_OK;
}

}  // namespace
}  // namespace hx

extern "C" int hx_fits_unpack_f64(int64_t nrows, int nc1, int nc2, int64_t s1, int64_t s2, int64_t srow, const void *table, double *array)
{
    return hx::fits_convert(true, nrows, nc1, nc2, s1, s2, srow, table, array);
}

extern "C" int hx_fits_pack_f64(int64_t nrows, int nc1, int nc2, int64_t s1, int64_t s2, int64_t srow, const double *array, void *table)
{
    return hx::fits_convert(false, nrows, nc1, nc2, s1, s2, srow, array, table);
}

extern "C" int hx_fits_unpack_columns(int64_t nrows, int64_t width, int ncols, const int64_t *offsets, const char *types, const double *tscal,
                                      const double *tzero, const void *table, double *const *columns, int flags)
{
    return hx::fits_unpack_columns(nrows, width, ncols, offsets, types, tscal, tzero, table, columns, flags);
}
