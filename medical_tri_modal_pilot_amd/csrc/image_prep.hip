// Chest X-ray input chain on the GPU: what the reference's loader does per image on CPU workers with PIL / torchvision
// (builder/data/dataset_new.py:2094-2096 F_t.equalize + self.transform, the chains of :91-160) -- histogram equalisation,
// antialiased bilinear resize, nearest-neighbour affine, centre crop, / 255 -- from the decoded uint8 pixels.
//
// The whole chain is integer arithmetic in PIL, so these kernels reproduce it bit for bit:
//   ImageOps.equalize   lut[i] = (step / 2 + sum_{j<i} h[j]) / step, step = (sum h - last non-zero h) / 255, saturated at 255;
//                       the identity when at most one bin is non-zero or step == 0
//   Image.resize        per axis clip8((sum pixel * k + 2^21) >> 22) with int32 weights k (22 fractional bits); the horizontal
//                       pass is rounded to uint8 before the vertical pass reads it
//   Image.transform     AFFINE / NEAREST in 16.16 fixed point: xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16,
//                       0 outside the source
//   ToTensor            float(byte) / 255 with IEEE division
// Sizes, weight tables, affine words and crop offsets come from the host in one int32 descriptor row per image
// (builder/data/cxr_transform.py, DESC_*); the images lie back to back in one uint8 buffer at arbitrary byte offsets.
// Three launches: the resized map goes through a uint8 scratch (80 KB per image at 256 x 311) -- a fused form would redo the
// horizontal pass once per vertical tap.
#include "common.hip.h"

namespace {

constexpr int DESC_WORDS = 24;
enum { D_SRC = 0, D_H, D_W, D_RH, D_RW, D_HB, D_HK, D_HKS, D_VB, D_VK, D_VKS, D_FLAGS, D_A0, D_A1, D_A2, D_A3, D_A4, D_A5, D_TOP,
       D_LEFT, D_SLOT, D_SCRATCH };
constexpr int HIST_CHUNK = 16384;                 // bytes of one image per workgroup of the histogram kernel
constexpr int TILE_ROWS = 32, TILE_COLS = 64;     // resized pixels per workgroup of the resize kernel
constexpr int PRECISION_BITS = 22;
constexpr int RESIZE_LDS_LIMIT = 60 * 1024;       // dynamic LDS (horizontal-pass rows); 2.3 KB more are static

MTMP_DEV int clip8(int v) { return min(max(v >> PRECISION_BITS, 0), 255); }

// 256-bin histograms.  Grid (chunks, images): a workgroup counts HIST_CHUNK bytes of its image into one LDS sub-histogram per wave
// and adds the non-empty bins to the global table: integer adds, so the result does not depend on the order.  16-byte loads
// between the first and the last 16-byte boundary of the chunk, single bytes at both ends.
__global__ __launch_bounds__(256) void cxr_hist_kernel(const uint8_t* __restrict__ pix, const int* __restrict__ desc,
                                                       unsigned* __restrict__ hist) {
    __shared__ unsigned sub[4][256];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int* d = desc + img * DESC_WORDS;
    const long long npx = (long long)d[D_H] * d[D_W];
    const long long begin = (long long)blockIdx.x * HIST_CHUNK;
    if (begin >= npx) return;
    const long long end = min(begin + HIST_CHUNK, npx);
    for (int i = tid; i < 4 * 256; i += 256) (&sub[0][0])[i] = 0u;
    __syncthreads();
    unsigned* mine = sub[tid >> 6];
    const uint8_t* b = pix + d[D_SRC] + begin;
    const uint8_t* e = pix + d[D_SRC] + end;
    const uint8_t* a0 = (const uint8_t*)(((uintptr_t)b + 15) & ~(uintptr_t)15);
    if (a0 > e) a0 = e;
    const uint8_t* a1 = a0 + ((e - a0) & ~(ptrdiff_t)15);
    if (b + tid < a0) atomicAdd(&mine[b[tid]], 1u);                     // at most 15 bytes
    for (const uint8_t* q = a0 + 16 * tid; q < a1; q += 16 * 256) {
        const uint4 v = *reinterpret_cast<const uint4*>(q);
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicAdd(&mine[wv[k] & 255u], 1u);
            atomicAdd(&mine[(wv[k] >> 8) & 255u], 1u);
            atomicAdd(&mine[(wv[k] >> 16) & 255u], 1u);
            atomicAdd(&mine[wv[k] >> 24], 1u);
        }
    }
    if (a1 + tid < e) atomicAdd(&mine[a1[tid]], 1u);                    // at most 15 bytes
    __syncthreads();
    const unsigned s = sub[0][tid] + sub[1][tid] + sub[2][tid] + sub[3][tid];
    if (s) atomicAdd(&hist[img * 256 + tid], s);
}

// Equalisation table + both resize passes.  Grid (column tiles, row tiles, images); a workgroup owns TILE_ROWS x TILE_COLS
// pixels of the resized map: it builds its image's table from the histogram (256-entry scan), runs the horizontal pass over the
// source rows its output rows read into LDS as uint8, then the vertical pass out of LDS.  Tables per axis: bounds int32
// [out][2] = (first source index, taps) and weights int32 [out][ksize].  in == out: one tap of 2^22, the pass is the identity.
__global__ __launch_bounds__(256) void cxr_resize_kernel(const uint8_t* __restrict__ pix, const int* __restrict__ desc,
                                                         const int* __restrict__ tab, const unsigned* __restrict__ hist,
                                                         uint8_t* __restrict__ scratch) {
    extern __shared__ uint8_t hrows[];            // [lds_rows of the launch][TILE_COLS]
    __shared__ unsigned scan[256], hraw[256];
    __shared__ uint8_t lut[256];
    __shared__ int last_nz;
    const int tid = threadIdx.x, img = blockIdx.z;
    const int* d = desc + img * DESC_WORDS;
    const int rh = d[D_RH], rw = d[D_RW], w = d[D_W];
    const int r0 = blockIdx.y * TILE_ROWS, c0 = blockIdx.x * TILE_COLS;
    if (r0 >= rh || c0 >= rw) return;             // the grid is sized for the largest map of the batch

    const unsigned hv = hist[img * 256 + tid];
    scan[tid] = hv;
    hraw[tid] = hv;
    if (tid == 0) last_nz = -1;
    __syncthreads();
    if (hv) atomicMax(&last_nz, tid);
    const int nz = __syncthreads_count(hv != 0u);
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned t = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += t;
        __syncthreads();
    }
    const unsigned step = nz > 1 ? (scan[255] - hraw[last_nz]) / 255u : 0u;
    lut[tid] = (uint8_t)(step ? min((step / 2u + (scan[tid] - hv)) / step, 255u) : (unsigned)tid);
    __syncthreads();

    const int* hb = tab + d[D_HB];
    const int* hk = tab + d[D_HK];
    const int* vb = tab + d[D_VB];
    const int* vk = tab + d[D_VK];
    const int hks = d[D_HKS], vks = d[D_VKS];
    const int r1 = min(r0 + TILE_ROWS, rh);
    const int y0 = vb[2 * r0];
    const int nrows = vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - y0;      // <= lds_rows: the caller's precondition (mtmp.h)
    const int c = tid & (TILE_COLS - 1), col = c0 + c;
    const bool live = col < rw;
    if (live) {
        const int x0 = hb[2 * col], n = hb[2 * col + 1];
        const int* k = hk + (long long)col * hks;
        const uint8_t* s0 = pix + d[D_SRC] + x0;
        for (int r = tid / TILE_COLS; r < nrows; r += 256 / TILE_COLS) {
            const uint8_t* s = s0 + (long long)(y0 + r) * w;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int j = 0; j < n; ++j) acc += (int)lut[s[j]] * k[j];
            hrows[r * TILE_COLS + c] = (uint8_t)clip8(acc);
        }
    }
    __syncthreads();
    if (live) {
        uint8_t* dst = scratch + d[D_SCRATCH];
        for (int r = r0 + tid / TILE_COLS; r < r1; r += 256 / TILE_COLS) {
            const int ya = vb[2 * r] - y0, n = vb[2 * r + 1];
            const int* k = vk + (long long)r * vks;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int j = 0; j < n; ++j) acc += (int)hrows[(ya + j) * TILE_COLS + c] * k[j];
            dst[(long long)r * rw + col] = (uint8_t)clip8(acc);
        }
    }
}

// Affine map + centre crop + / 255.  Grid (pixel blocks, output slots); slot_map[slot] = image or -1: a slot without an image is
// written as zeros by the same launch (the reference's torch.zeros(image_size)).
__global__ __launch_bounds__(256) void cxr_affine_crop_kernel(const uint8_t* __restrict__ scratch, const int* __restrict__ desc,
                                                              const int* __restrict__ slot_map, float* __restrict__ out, int S) {
    const int slot = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * S) return;
    const int img = slot_map[slot];
    float v = 0.0f;
    if (img >= 0) {
        const int* d = desc + img * DESC_WORDS;
        const int rh = d[D_RH], rw = d[D_RW];
        int y = i / S + d[D_TOP], x = i % S + d[D_LEFT];
        if (d[D_FLAGS] & 1) {
            const int xin = (d[D_A2] + d[D_A0] * x + d[D_A1] * y) >> 16;
            const int yin = (d[D_A5] + d[D_A3] * x + d[D_A4] * y) >> 16;
            x = xin;
            y = yin;
        }
        if (x >= 0 && x < rw && y >= 0 && y < rh) v = __fdiv_rn((float)scratch[d[D_SCRATCH] + (long long)y * rw + x], 255.0f);
    }
    out[(long long)slot * S * S + i] = v;
}

}  // namespace

extern "C" int mtmp_cxr_hist(const uint8_t* pixels, const int32_t* desc, uint32_t* hist, int n, int max_pixels, void* stream) {
    MTMP_CHECK_ARG(pixels && desc && hist && n > 0 && n <= 65535 && max_pixels > 0,
                   "mtmp_cxr_hist: bad argument (n=%d max_pixels=%d)", n, max_pixels);
    const int chunks = (max_pixels + HIST_CHUNK - 1) / HIST_CHUNK;
    hipLaunchKernelGGL(cxr_hist_kernel, dim3(chunks, n), dim3(256), 0, (hipStream_t)stream, pixels, desc, hist);
    MTMP_CHECK_LAUNCH("mtmp_cxr_hist");
    return MTMP_OK;
}

extern "C" int mtmp_cxr_resize(const uint8_t* pixels, const int32_t* desc, const int32_t* tables, const uint32_t* hist,
                               uint8_t* scratch, int n, int max_rh, int max_rw, int lds_rows, void* stream) {
    MTMP_CHECK_ARG(pixels && desc && tables && hist && scratch && n > 0 && n <= 65535 && max_rh > 0 && max_rw > 0 && lds_rows > 0,
                   "mtmp_cxr_resize: bad argument (n=%d max_rh=%d max_rw=%d lds_rows=%d)", n, max_rh, max_rw, lds_rows);
    MTMP_CHECK_ARG((long long)lds_rows * TILE_COLS <= RESIZE_LDS_LIMIT && (max_rh + TILE_ROWS - 1) / TILE_ROWS <= 65535,
                   "mtmp_cxr_resize: %d source rows per tile of %d resized rows exceed the LDS budget of %d rows (or max_rh=%d "
                   "is too large)", lds_rows, TILE_ROWS, RESIZE_LDS_LIMIT / TILE_COLS, max_rh);
    const dim3 grid((max_rw + TILE_COLS - 1) / TILE_COLS, (max_rh + TILE_ROWS - 1) / TILE_ROWS, n);
    hipLaunchKernelGGL(cxr_resize_kernel, grid, dim3(256), (size_t)lds_rows * TILE_COLS, (hipStream_t)stream, pixels, desc, tables,
                       hist, scratch);
    MTMP_CHECK_LAUNCH("mtmp_cxr_resize");
    return MTMP_OK;
}

extern "C" int mtmp_cxr_affine_crop(const uint8_t* scratch, const int32_t* desc, const int32_t* slot_map, float* out, int n_slots,
                                    int S, void* stream) {
    MTMP_CHECK_ARG(scratch && desc && slot_map && out && n_slots > 0 && n_slots <= 65535 && S > 0 && S <= 4096 &&
                       (long long)n_slots * S * S < (1ll << 31),
                   "mtmp_cxr_affine_crop: bad argument (n_slots=%d S=%d)", n_slots, S);
    hipLaunchKernelGGL(cxr_affine_crop_kernel, dim3((S * S + 255) / 256, n_slots), dim3(256), 0, (hipStream_t)stream, scratch, desc,
                       slot_map, out, S);
    MTMP_CHECK_LAUNCH("mtmp_cxr_affine_crop");
    return MTMP_OK;
}
