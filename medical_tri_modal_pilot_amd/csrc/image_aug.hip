// The random chest X-ray input chains on the GPU: --image-train-type random (RandomResizedCrop) and randaug (RandAugment in
// front of it), builder/data/dataset_new.py:60-89 of the reference, from the decoded uint8 pixels.  Per image: equalise, the
// two RandAugment ops, the crop box, PIL's two-pass antialiased bilinear resize of the box to S x S, / 255.
//
// Everything PIL does here is integer, table or correctly rounded float arithmetic, reproduced bit for bit:
//   table ops     Equalize (ImageOps.equalize, see image_prep.hip), AutoContrast (int(v * s - lo * s), s = 255.0 / (hi - lo) in
//                 doubles, clipped; identity when hi <= lo), Brightness / Contrast (Image.blend of the constant 0 / int(mean + .5)
//                 with the image), Posterize (v & mask), Solarize (v < t ? v : 255 - v).  No pass over the pixels: the kernel that
//                 next READS the image composes the pending tables in its prologue, from the 256-bin histogram of what it reads,
//                 pushing the counts through each table so that a later Contrast / AutoContrast / Equalize sees the right ones.
//   Image.blend   a + f * (b - a) in float32, the product rounded before the sum, clipped to [0, 255], truncated
//   stages        ops that move or mix pixels write a full-size uint8 map: the 16.16 nearest-neighbour affine map of
//                 Image.transform (shears, rotation; a translation is the same words), 0 outside the source; Sharpness = blend of
//                 ImageFilter.SMOOTH ((1 1 1 / 1 5 1 / 1 1 1) / 13 rounded half up, border copied) with the image.  A stage reads
//                 its source through the pending table and counts the histogram of what it writes.
//   resize        the window (i, j, ch, cw) of the last map through the pending table, horizontal pass rounded to uint8 in LDS,
//                 vertical pass out of LDS, float(byte) / 255 with IEEE division straight into the image's S x S slot.
// Plan: one int32 row of AUG_WORDS per image from builder/data/cxr_transform.py (AUG_*).
#include "common.hip.h"

namespace {

constexpr int AUG_WORDS = 64;
enum { A_SRC = 0, A_H, A_W, A_SLOT, A_SCR, A_I, A_J, A_CH, A_CW, A_HB, A_HK, A_HKS, A_VB, A_VK, A_VKS };
constexpr int A_STAGE = 16, A_READ = 32;          // + 8 k / + 8 r
enum { STAGE_NONE = 0, STAGE_AFFINE = 1, STAGE_SHARPNESS = 2 };
enum { T_EQUALIZE = 1, T_BRIGHTNESS, T_CONTRAST, T_POSTERIZE, T_SOLARIZE, T_AUTOCONTRAST };
constexpr int STAGE_PX = 4096;                    // pixels of one image per workgroup of the stage kernel: 4 x 4 per thread
constexpr int TILE_ROWS = 32, TILE_COLS = 64;     // output pixels per workgroup of the resize kernel
constexpr int PRECISION_BITS = 22;
constexpr int RESIZE_LDS_LIMIT = 60 * 1024;       // dynamic LDS (horizontal-pass rows); 3.6 KB more are static

MTMP_DEV int clip8(int v) { return min(max(v >> PRECISION_BITS, 0), 255); }

// Image.blend(a, b, f) for one pixel: two float32 roundings (no fused multiply-add), clip, truncate.
MTMP_DEV unsigned blend8(int a, int b, float f) {
#pragma clang fp contract(off)
    const float p = f * (float)(b - a);
    const float t = (float)a + p;
    return (unsigned)(int)fminf(fmaxf(t, 0.0f), 255.0f);
}

// ImageOps.autocontrast's table entry: Python floats, every operation rounded on its own.
MTMP_DEV unsigned autocontrast8(int v, int lo, int hi) {
#pragma clang fp contract(off)
    const double scale = 255.0 / (double)(hi - lo);
    const double offset = -(double)lo * scale;
    const double p = (double)v * scale;
    const double t = p + offset;
    return (unsigned)min(max((int)t, 0), 255);
}

struct LutShared {
    unsigned h[256], h2[256], scan[256];
    unsigned long long sum;
    int lo, hi;
    uint8_t lut[256], tb[256];
};

// s.lut <- the composition of reader `rd`'s pending table ops (rd = the 8 words base, count, 3 codes, 3 parameters), from the
// histogram of the reader's base map (hist uint32 [3][n][256]: source pixels, map of stage 0, map of stage 1).  All 256 threads.
MTMP_DEV void build_lut(const int* rd, const unsigned* __restrict__ hist, int n, int img, LutShared& s) {
    const int tid = threadIdx.x, nt = min(rd[1], 3);
    s.lut[tid] = (uint8_t)tid;
    s.h[tid] = nt > 0 ? hist[((long long)rd[0] * n + img) * 256 + tid] : 0u;
    __syncthreads();
    for (int t = 0; t < nt; ++t) {                // the op codes are uniform over the workgroup
        const int code = rd[2 + t], par = rd[5 + t];
        const unsigned hv = s.h[tid];
        s.scan[tid] = hv;
        s.h2[tid] = 0u;
        if (tid == 0) { s.lo = 256; s.hi = -1; s.sum = 0ull; }
        __syncthreads();
        if (hv) {
            atomicMin(&s.lo, tid);
            atomicMax(&s.hi, tid);
            atomicAdd(&s.sum, (unsigned long long)hv * (unsigned)tid);
        }
        const int nz = __syncthreads_count(hv != 0u);
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned v = tid >= off ? s.scan[tid - off] : 0u;
            __syncthreads();
            s.scan[tid] += v;
            __syncthreads();
        }
        const unsigned total = s.scan[255];
        const int lo = s.lo, hi = s.hi;
        unsigned e = (unsigned)tid;
        if (code == T_EQUALIZE) {
            const unsigned step = nz > 1 ? (total - s.h[hi]) / 255u : 0u;
            if (step) e = min((step / 2u + (s.scan[tid] - hv)) / step, 255u);
        } else if (code == T_BRIGHTNESS) {
            e = blend8(0, tid, __int_as_float(par));
        } else if (code == T_CONTRAST) {
            const int mean = total ? (int)((2ull * s.sum + total) / (2ull * total)) : 0;       // int(sum / total + 0.5)
            e = blend8(mean, tid, __int_as_float(par));
        } else if (code == T_POSTERIZE) {
            e = (unsigned)(tid & par);
        } else if (code == T_SOLARIZE) {
            e = (unsigned)(tid < par ? tid : 255 - tid);
        } else if (code == T_AUTOCONTRAST) {
            if (hi > lo) {
                e = autocontrast8(tid, lo, hi);
            }
        }
        s.tb[tid] = (uint8_t)e;
        __syncthreads();
        if (hv) atomicAdd(&s.h2[e], hv);
        s.lut[tid] = s.tb[s.lut[tid]];
        __syncthreads();
        s.h[tid] = s.h2[tid];
        __syncthreads();
    }
}

MTMP_DEV const uint8_t* base_map(const int* d, int base, const uint8_t* pix, const uint8_t* scratch, long long half_bytes) {
    return base == 0 ? pix + d[A_SRC] : scratch + (long long)(base - 1) * half_bytes + d[A_SCR];
}

// One RandAugment op that writes a map.  Grid (chunks of STAGE_PX pixels, images); images whose op `stage` is a table op or nothing
// return at once.  Reads the op's base map through the pending table, writes map `stage` (scratch half `stage`, 16-byte aligned
// per image: four pixels per 32-bit store) and adds the histogram of what it wrote to hist[1 + stage][img].
__global__ __launch_bounds__(256) void cxr_aug_stage_kernel(const uint8_t* __restrict__ pix, const int* __restrict__ aug,
                                                            unsigned* __restrict__ hist, uint8_t* __restrict__ scratch, int n,
                                                            long long half_bytes, int stage) {
    __shared__ LutShared s;
    __shared__ unsigned sub[256];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int* d = aug + img * AUG_WORDS;
    const int* st = d + A_STAGE + 8 * stage;
    const int kind = st[0];
    const int h = d[A_H], w = d[A_W], npx = h * w;
    const int begin = blockIdx.x * STAGE_PX;
    if (kind == STAGE_NONE || begin >= npx) return;
    const int* rd = d + A_READ + 8 * stage;
    build_lut(rd, hist, n, img, s);
    sub[tid] = 0u;
    __syncthreads();
    const uint8_t* src = base_map(d, rd[0], pix, scratch, half_bytes);
    uint8_t* dst = scratch + (long long)stage * half_bytes + d[A_SCR];
    const int a0 = st[1], a1 = st[2], a2 = st[3], a3 = st[4], a4 = st[5], a5 = st[6];
    const float factor = __int_as_float(st[1]);
#pragma unroll 1
    for (int g = 0; g < STAGE_PX / 1024; ++g) {
        const int p0 = begin + (g * 256 + tid) * 4;
        if (p0 >= npx) break;
        int y = p0 / w, x = p0 - y * w;
        unsigned packed = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p0 + k < npx) {
                unsigned v = 0u;
                if (kind == STAGE_AFFINE) {
                    const int xin = (a2 + a0 * x + a1 * y) >> 16, yin = (a5 + a3 * x + a4 * y) >> 16;
                    if (xin >= 0 && xin < w && yin >= 0 && yin < h) v = s.lut[src[(long long)yin * w + xin]];
                } else {
                    const uint8_t* c = src + (long long)y * w + x;
                    const int ctr = s.lut[c[0]];
                    v = (unsigned)ctr;
                    if (x > 0 && y > 0 && x < w - 1 && y < h - 1) {
                        const int t = 5 * ctr + s.lut[c[-w - 1]] + s.lut[c[-w]] + s.lut[c[-w + 1]] + s.lut[c[-1]] + s.lut[c[1]] +
                                      s.lut[c[w - 1]] + s.lut[c[w]] + s.lut[c[w + 1]];
                        v = blend8((2 * t + 13) / 26, ctr, factor);
                    }
                }
                packed |= v << (8 * k);
                atomicAdd(&sub[v], 1u);
                if (++x == w) { x = 0; ++y; }
            }
        }
        if (p0 + 3 < npx) {
            *reinterpret_cast<unsigned*>(dst + p0) = packed;
        } else {
            for (int k = 0; p0 + k < npx; ++k) dst[p0 + k] = (uint8_t)(packed >> (8 * k));
        }
    }
    __syncthreads();
    if (sub[tid]) atomicAdd(&hist[((long long)(1 + stage) * n + img) * 256 + tid], sub[tid]);
}

// Crop box + both resize passes + / 255.  Grid (column tiles, row tiles, output slots) of the S x S outputs; slot_map[slot] = image
// or -1: a slot without an image is written as zeros by the same launch.  A workgroup owns TILE_ROWS x TILE_COLS output pixels:
// the pending table in its prologue, the horizontal pass over the box rows its output rows read into LDS as uint8, the vertical
// pass out of LDS.  Tables per axis as in image_prep.hip, built for (cw -> S) and (ch -> S): indices are relative to the box.
__global__ __launch_bounds__(256) void cxr_crop_resize_kernel(const uint8_t* __restrict__ pix, const uint8_t* __restrict__ scratch,
                                                              const int* __restrict__ aug, const int* __restrict__ tab,
                                                              const unsigned* __restrict__ hist, const int* __restrict__ slot_map,
                                                              float* __restrict__ out, int n, int S, long long half_bytes,
                                                              int lds_rows) {
    extern __shared__ __attribute__((aligned(16))) uint8_t hrows[];          // [lds_rows][TILE_COLS]
    __shared__ LutShared s;
    const int tid = threadIdx.x, slot = blockIdx.z;
    const int r0 = blockIdx.y * TILE_ROWS, c0 = blockIdx.x * TILE_COLS;
    const int r1 = min(r0 + TILE_ROWS, S);
    const int c = tid & (TILE_COLS - 1), col = c0 + c;
    const bool live = col < S;
    float* o = out + (long long)slot * S * S;
    const int img = slot_map[slot];
    if (img < 0 || img >= n) {
        if (live)
            for (int r = r0 + tid / TILE_COLS; r < r1; r += 256 / TILE_COLS) o[r * S + col] = 0.0f;
        return;
    }
    const int* d = aug + img * AUG_WORDS;
    const int* rd = d + A_READ + 16;
    build_lut(rd, hist, n, img, s);
    const uint8_t* src = base_map(d, rd[0], pix, scratch, half_bytes);
    const int w = d[A_W];
    const int* hb = tab + d[A_HB];
    const int* hk = tab + d[A_HK];
    const int* vb = tab + d[A_VB];
    const int* vk = tab + d[A_VK];
    const int hks = d[A_HKS], vks = d[A_VKS];
    const int y0 = vb[2 * r0];
    const int nrows = min(vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - y0, lds_rows);       // never past the LDS rows of the launch
    if (live) {
        const int x0 = hb[2 * col], nt = hb[2 * col + 1];
        const int* k = hk + (long long)col * hks;
        const uint8_t* s0 = src + (long long)(d[A_I] + y0) * w + d[A_J] + x0;
        for (int r = tid / TILE_COLS; r < nrows; r += 256 / TILE_COLS) {
            const uint8_t* p = s0 + (long long)r * w;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int j = 0; j < nt; ++j) acc += (int)s.lut[p[j]] * k[j];
            hrows[r * TILE_COLS + c] = (uint8_t)clip8(acc);
        }
    }
    __syncthreads();
    if (live) {
        for (int r = r0 + tid / TILE_COLS; r < r1; r += 256 / TILE_COLS) {
            const int ya = vb[2 * r] - y0, nt = min(vb[2 * r + 1], nrows - ya);
            const int* k = vk + (long long)r * vks;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int j = 0; j < nt; ++j) acc += (int)hrows[(ya + j) * TILE_COLS + c] * k[j];
            o[r * S + col] = __fdiv_rn((float)clip8(acc), 255.0f);
        }
    }
}

}  // namespace

extern "C" int mtmp_cxr_aug_stage(const uint8_t* pixels, const int32_t* aug, uint32_t* hist, uint8_t* scratch, int n, int max_pixels,
                                  long long half_bytes, int stage, void* stream) {
    MTMP_CHECK_ARG(pixels && aug && hist && scratch && n > 0 && n <= 65535 && max_pixels > 0 && (stage == 0 || stage == 1) &&
                       half_bytes > 0 && half_bytes % 16 == 0 && ((uintptr_t)scratch & 15) == 0,
                   "mtmp_cxr_aug_stage: bad argument (n=%d max_pixels=%d half_bytes=%lld stage=%d)", n, max_pixels, half_bytes, stage);
    const int chunks = (max_pixels + STAGE_PX - 1) / STAGE_PX;
    hipLaunchKernelGGL(cxr_aug_stage_kernel, dim3(chunks, n), dim3(256), 0, (hipStream_t)stream, pixels, aug, hist, scratch, n,
                       half_bytes, stage);
    MTMP_CHECK_LAUNCH("mtmp_cxr_aug_stage");
    return MTMP_OK;
}

extern "C" int mtmp_cxr_crop_resize(const uint8_t* pixels, const uint8_t* scratch, const int32_t* aug, const int32_t* tables,
                                    const uint32_t* hist, const int32_t* slot_map, float* out, int n, int n_slots, int S,
                                    long long half_bytes, int lds_rows, void* stream) {
    MTMP_CHECK_ARG(pixels && scratch && aug && tables && hist && slot_map && out && n >= 0 && n <= 65535 && n_slots > 0 &&
                       n_slots <= 65535 && S > 0 && S <= 4096 && (long long)n_slots * S * S < (1ll << 31) && half_bytes >= 0 &&
                       lds_rows > 0,
                   "mtmp_cxr_crop_resize: bad argument (n=%d n_slots=%d S=%d half_bytes=%lld lds_rows=%d)", n, n_slots, S, half_bytes,
                   lds_rows);
    MTMP_CHECK_ARG((long long)lds_rows * TILE_COLS <= RESIZE_LDS_LIMIT,
                   "mtmp_cxr_crop_resize: %d box rows per tile of %d output rows exceed the LDS budget of %d rows", lds_rows,
                   TILE_ROWS, RESIZE_LDS_LIMIT / TILE_COLS);
    const dim3 grid((S + TILE_COLS - 1) / TILE_COLS, (S + TILE_ROWS - 1) / TILE_ROWS, n_slots);
    hipLaunchKernelGGL(cxr_crop_resize_kernel, grid, dim3(256), (size_t)lds_rows * TILE_COLS, (hipStream_t)stream, pixels, scratch,
                       aug, tables, hist, slot_map, out, n, S, half_bytes, lds_rows);
    MTMP_CHECK_LAUNCH("mtmp_cxr_crop_resize");
    return MTMP_OK;
}
