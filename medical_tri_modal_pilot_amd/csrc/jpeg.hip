// Baseline greyscale JPEG decoding on the GPU: what the reference's loader does per image with PIL's Image.open
// (builder/data/dataset_new.py:2094) on files PIL wrote (1_mimic_cxr_preprocess.py:81-82: 8-bit, one component, baseline
// sequential, Huffman coded).  There is no colour conversion, no upsampling and no float, so the pixels equal PIL's bit for bit.
// The host (builder/data/jpeg.py) parses the markers, takes the stuffed FF 00 pairs and the RSTn markers out of the
// entropy-coded bytes and hands over one int32 row per image (JPG_*), one per restart segment (SEG_*), and the tables.
//
// mtmp_jpeg_entropy   one workgroup per segment, one lane per subsequence of `subseq_bits` bits.  Every lane runs ONE device
//   function, span(): decode from a state (bit position; coefficient index 0..63, 0 = a DC code is next) up to the first symbol
//   that starts at or behind the subsequence's end, return the exit state, the blocks completed and the sum of their DC
//   differences.  Lanes synchronise themselves the way the published parallel Huffman decoders do: all decode from their nominal
//   start as if a block began there; then, round by round, every lane whose left neighbour's exit state moved decodes again from
//   it, until a round moves no exit state.  Lane 0 is right by construction, so after r rounds lanes 0..r are: the rounds are
//   bounded by the number of subsequences.  A scan of block counts and DC sums gives every lane its first block and its DC
//   predictor, and a last span() call writes the coefficients (int16, natural order, DC absolute) into the zeroed buffer.
//   Every loop here is bounded by a launch argument or a descriptor word: span() moves on by at least one bit per turn (a code
//   that is not in the table, or a symbol that would end behind the segment, costs one bit), the slow path of the code lookup
//   walks lengths 11..16, the rounds stop at the lane count.  Nothing waits for another workgroup.  Bits behind the segment's end
//   read as ones: no code is all ones, so the fill bits and the end of a truncated stream are not symbols.
// mtmp_jpeg_sync_points    the same kernel under a template flag, once per file when an image store is built
//   (builder/data/cxr_store.py): what the rounds and the scan find -- every lane's entry state, first block and DC predictor --
//   is a property of the file, so it is written to a sync table in place of the write pass.
// mtmp_jpeg_store_entropy  the per-batch decoder of such a store: a flat grid over the batch's subsequences, each lane ONE span()
//   call from its sync row.  No rounds, no scan, no per-segment workgroup.
// mtmp_jpeg_idct      eight lanes per block: a column per lane, the transpose through LDS, a row per lane.  Dequantisation and
//   both passes of libjpeg's jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2, its twelve FIX constants), which PIL's
//   libjpeg-turbo computes bit-identically in its SIMD forms; the library's zero-AC shortcuts equal the general path, so there
//   is none here.  The arithmetic is done on unsigned words (wrapping), so a corrupt stream cannot overflow a signed int.
#include "common.hip.h"

namespace {

constexpr int JPG_WORDS = 16, SEG_WORDS = 4;
enum { J_STREAM = 0, J_SEG0, J_NSEG, J_H, J_W, J_BPR, J_NBLK, J_DST, J_QT, J_DC, J_AC, J_COEF, J_RI, J_SUBSEQ, J_NSYNC };
enum { S_OFF = 0, S_BYTES, S_IMG, S_BLOCK0 };
enum { T_OFF = 0, T_BYTES, T_BLOCK0, T_SYNC0 };    // a segment row of the image store: everything relative to its image
enum { W_STREAM = 0, W_SYNC0 };                    // the two 64-bit words of a stored image
constexpr int LOOK_BITS = 10, LOOK = 1 << LOOK_BITS;
constexpr int HUFF_WORDS = LOOK + 18 + 18 + 256;   // look | maxcode[18] | valoff[18] | huffval[256]  (builder/data/jpeg.py)
constexpr int MAX_SUBSEQ = 1024;                   // lanes of a workgroup
constexpr int MAX_SEGMENT_BYTES = 1 << 22;         // (bit position << 6 | coefficient index) is one 32-bit state word
constexpr int MAX_STAGE_BYTES = 32 * 1024;         // dynamic LDS: a segment up to the launch's stage_bytes is decoded out of it
constexpr int STATUS_SHORT = 1, STATUS_LANES = 2, STATUS_SEGMENTS = 4;

__constant__ uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct SpanOut {
    int p, k, nblk, dcs;
};

// 32 bits of the segment from bit p on; bits behind its end read as ones
MTMP_DEV unsigned window(const uint8_t* seg, int nbytes, int p) {
    const int b = p >> 3;
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) v = (v << 8) | (b + i < nbytes ? (unsigned)seg[b + i] : 0xFFu);
    return (unsigned)(v >> (8 - (p & 7)));
}

// From state (p, k) up to the first symbol that starts at or behind `end`.  WRITE: the coefficients of blocks blk.. < nb go to
// coef (the segment's first block), DC = pred + the running sum of differences.  zz: the ZIGZAG table the write pass reads (the
// constant itself, or a workgroup's LDS copy of it: the read sits in front of every coefficient's store).
template <bool WRITE>
MTMP_DEV SpanOut span(const uint8_t* seg, int nbytes, int nbits, const int* dc, const int* ac, int p, int k, int end,
                      int16_t* coef, int blk, int pred, int nb, const uint8_t* zz = ZIGZAG) {
    int nblk = 0, dcs = 0;
    while (p < end) {                              // p grows by at least one per turn
        const unsigned win = window(seg, nbytes, p);
        const int* t = k ? ac : dc;
        const int e = t[win >> (32 - LOOK_BITS)];
        int len = e >> 8, sym = e & 255;
        if (e == 0) {
            const int code16 = (int)(win >> 16);
            for (int l = LOOK_BITS + 1; l <= 16; ++l) {
                const int code = code16 >> (16 - l);
                if (code <= t[LOOK + l]) {
                    len = l;
                    sym = t[LOOK + 36 + ((code + t[LOOK + 18 + l]) & 255)];
                    break;
                }
            }
        }
        const int s = sym & 15;
        if (len == 0 || p + len + s > nbits) {     // no such code, or the symbol would end behind the data
            p += 1;
            continue;
        }
        int v = 0;
        if (s) {
            v = (int)((win >> (32 - len - s)) & ((1u << s) - 1u));
            if (v < (1 << (s - 1))) v -= (1 << s) - 1;
        }
        p += len + s;
        if (k == 0) {
            dcs += v;
            pred += v;
            if (WRITE && blk < nb) coef[(long long)blk * 64] = (int16_t)pred;
            k = 1;
        } else {
            const int r = sym >> 4;
            if (s == 0) {
                k = r == 15 ? k + 16 : 64;         // ZRL | EOB
            } else {
                k += r;
                if (WRITE && k < 64 && blk < nb) coef[(long long)blk * 64 + zz[k]] = (int16_t)v;
                k += 1;
            }
        }
        if (k >= 64) {
            k = 0;
            ++nblk;
            ++blk;
        }
    }
    return SpanOut{p, k, nblk, dcs};
}

// SYNC: the build pass of the image store (mtmp_jpeg_sync_points).  The same rounds and the same scan; what a lane has found --
// its entry state, its first block, its DC predictor -- goes to its row of the sync table in place of the write pass, and the
// subsequence length is the image's own (J_SUBSEQ).  sync0[sid]: the segment's first row; rows >= n_sync are not written.
template <bool SYNC>
__global__ __launch_bounds__(MAX_SUBSEQ) void jpeg_entropy_kernel(const uint8_t* __restrict__ streams,
                                                                  const int* __restrict__ desc, const int* __restrict__ segs,
                                                                  const int* __restrict__ tables, int16_t* __restrict__ coef,
                                                                  int* __restrict__ status, int* __restrict__ rounds_out,
                                                                  int subseq_bits, int stage_bytes, const int* __restrict__ sync0,
                                                                  int4* __restrict__ sync, long long n_sync) {
    __shared__ int tab[2][HUFF_WORDS];             // 10.3 KB
    __shared__ unsigned exit_s[MAX_SUBSEQ];        // 4 KB
    __shared__ int nblk_s[MAX_SUBSEQ], dcs_s[MAX_SUBSEQ];        // 8 KB
    extern __shared__ uint8_t stage[];             // stage_bytes <= 32 KB: at most 54.3 KB in all
    const int tid = threadIdx.x, nthr = blockDim.x, sid = blockIdx.x;
    const int* sg = segs + (long long)sid * SEG_WORDS;
    const int img = sg[S_IMG], b0 = sg[S_BLOCK0];
    const int* d = desc + (long long)img * JPG_WORDS;
    const int nbytes = min(max(sg[S_BYTES], 0), MAX_SEGMENT_BYTES), nbits = nbytes * 8;
    const int ri = d[J_RI], left = d[J_NBLK] - b0;
    const int nb = max(ri > 0 ? min(ri, left) : left, 0);
    const int S = SYNC ? max(d[J_SUBSEQ], 1) : subseq_bits > 0 ? subseq_bits : max(nbits, 1);
    const int nsub = (int)max(((long long)nbits + S - 1) / S, 1ll);
    if (nsub > nthr) {                             // uniform: the host cut the segments for this launch's lane count
        if (tid == 0) atomicOr(&status[img], STATUS_LANES);
        return;
    }
    for (int i = tid; i < HUFF_WORDS; i += nthr) {
        tab[0][i] = tables[d[J_DC] + i];
        tab[1][i] = tables[d[J_AC] + i];
    }
    const uint8_t* seg = streams + sg[S_OFF];
    if (nbytes <= stage_bytes) {
        for (int i = tid; i < nbytes; i += nthr) stage[i] = seg[i];
        seg = stage;
    }
    __syncthreads();

    const bool active = tid < nsub;
    const int end = active ? min((tid + 1) * S, nbits) : 0;
    unsigned used = active ? (unsigned)(tid * S) << 6 : 0u;        // the entry state this lane decoded from last
    SpanOut r{0, 0, 0, 0};
    if (active) r = span<false>(seg, nbytes, nbits, tab[0], tab[1], tid * S, 0, end, nullptr, 0, 0, 0);
    exit_s[tid] = ((unsigned)r.p << 6) | (unsigned)r.k;
    __syncthreads();
    int rounds = 1;
    for (int round = 1; round < nsub; ++round) {
        const unsigned entry = (active && tid > 0) ? exit_s[tid - 1] : used;
        __syncthreads();
        int changed = 0;
        if (entry != used) {
            used = entry;
            r = span<false>(seg, nbytes, nbits, tab[0], tab[1], (int)(entry >> 6), (int)(entry & 63u), end, nullptr, 0, 0, 0);
            const unsigned ex = ((unsigned)r.p << 6) | (unsigned)r.k;
            changed = ex != exit_s[tid];
            exit_s[tid] = ex;
        }
        if (!__syncthreads_or(changed)) break;
        ++rounds;
    }

    nblk_s[tid] = active ? r.nblk : 0;
    dcs_s[tid] = active ? r.dcs : 0;
    __syncthreads();
    for (int off = 1; off < nthr; off <<= 1) {
        const int a = tid >= off ? nblk_s[tid - off] : 0, b = tid >= off ? dcs_s[tid - off] : 0;
        __syncthreads();
        nblk_s[tid] += a;
        dcs_s[tid] += b;
        __syncthreads();
    }
    if (active) {
        const int blk0 = tid ? nblk_s[tid - 1] : 0, pred = tid ? dcs_s[tid - 1] : 0;
        if (SYNC) {
            const long long row = (long long)sync0[sid] + tid;
            if (row >= 0 && row < n_sync) sync[row] = int4{(int)used, blk0, pred, sid - d[J_SEG0]};
        } else {
            span<true>(seg, nbytes, nbits, tab[0], tab[1], (int)(used >> 6), (int)(used & 63u), end,
                       coef + ((long long)d[J_COEF] + b0) * 64, blk0, pred, nb);
        }
    }
    if (tid == 0) {
        int code = nblk_s[nsub - 1] < nb ? STATUS_SHORT : 0;
        if (sid - d[J_SEG0] == d[J_NSEG] - 1 && b0 + nb < d[J_NBLK]) code |= STATUS_SEGMENTS;
        if (code) atomicOr(&status[img], code);
        if (rounds_out) rounds_out[sid] = rounds;
    }
}

constexpr int STORE_LANES = 256;
constexpr int STORE_STAGE_BITS = 1024;                           // a subsequence of up to this many bits is decoded out of LDS
constexpr int STORE_STAGE_WORDS = STORE_STAGE_BITS / 32 + 1;     // + 4 bytes: the last symbol's window; 33 words: no bank conflicts
#ifndef MTMP_JPEG_STORE_TABLES_LDS
#define MTMP_JPEG_STORE_TABLES_LDS 1                             // 0: every lane reads its tables from global memory (the A/B of
#endif                                                           // profiles/cxr_store.txt; a diagnostic build only)

// The per-batch decoder of the image store: a flat grid over the subsequences of the batch's images, one lane each, ONE span()
// call from the stored entry state.  prefix[b] = lanes of the batch's images < b; a lane finds its image by bisection (at most
// 32 turns), its segment through its sync row.  The decode tables of the workgroup's first image are copied into LDS; a lane
// whose image names another pair reads its own from global memory (a wave-uniform choice wherever a wave holds one image).
// The 64 bytes of ZIGZAG are copied with them.  A lane whose subsequence has at most STORE_STAGE_BITS bits (the default length) first copies its bytes -- 33 independent
// loads -- into LDS words of its own and decodes from there with all positions rebased to its subsequence: span() then waits
// for LDS, not for global memory, once per symbol.  The words are the lane's alone, so no barrier follows the table load.
// Every index that comes out of a row is checked against the size of what it indexes before it is used.
__global__ __launch_bounds__(STORE_LANES) void jpeg_store_entropy_kernel(
    const uint8_t* __restrict__ streams, const int* __restrict__ segs, const int4* __restrict__ sync,
    const int* __restrict__ tables, const int* __restrict__ desc, const long long* __restrict__ wide,
    const int* __restrict__ prefix, int16_t* __restrict__ coef, int n, int total, long long stream_bytes, long long n_segs,
    long long n_sync, long long table_words) {
    __shared__ int tab[2][HUFF_WORDS];             // 10.3 KB
    __shared__ unsigned stage[STORE_LANES * STORE_STAGE_WORDS];  // 33 KB
    __shared__ uint8_t zz[64];
    const int tid = threadIdx.x, g = blockIdx.x * STORE_LANES + tid;
    auto image_of = [&](int lane) {                // the last b with prefix[b] <= lane
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= lane) lo = mid; else hi = mid;
        }
        return lo;
    };
    const int* d0 = desc + (long long)image_of(min(blockIdx.x * STORE_LANES, total - 1)) * JPG_WORDS;
    const int dc0 = d0[J_DC], ac0 = d0[J_AC];
    const bool ok0 = MTMP_JPEG_STORE_TABLES_LDS && dc0 >= 0 && ac0 >= 0 && dc0 + HUFF_WORDS <= table_words &&
                     ac0 + HUFF_WORDS <= table_words;
    if (tid < 64) zz[tid] = ZIGZAG[tid];
    if (ok0)
        for (int i = tid; i < HUFF_WORDS; i += STORE_LANES) {
            tab[0][i] = tables[dc0 + i];
            tab[1][i] = tables[ac0 + i];
        }
    __syncthreads();
    if (g >= total) return;
    const int b = image_of(g), l = g - prefix[b];
    const int* d = desc + (long long)b * JPG_WORDS;
    const long long row = wide[2 * b + W_SYNC0] + l;
    if (l < 0 || l >= d[J_NSYNC] || row < 0 || row >= n_sync) return;
    const int4 sy = sync[row];                     // entry state, first block, DC predictor, segment
    const long long srow = (long long)d[J_SEG0] + sy.w;
    if (sy.w < 0 || sy.w >= d[J_NSEG] || srow < 0 || srow >= n_segs || sy.y < 0) return;
    const int* sg = segs + srow * SEG_WORDS;
    const int nbytes = min(max(sg[T_BYTES], 0), MAX_SEGMENT_BYTES), nbits = nbytes * 8;
    const long long soff = wide[2 * b + W_STREAM] + sg[T_OFF];
    const int j = l - sg[T_SYNC0], S = d[J_SUBSEQ], b0 = sg[T_BLOCK0];
    const int dc = d[J_DC], ac = d[J_AC];
    if (soff < 0 || soff + nbytes > stream_bytes || j < 0 || S < 1 || b0 < 0 || dc < 0 || ac < 0 ||
        dc + HUFF_WORDS > table_words || ac + HUFF_WORDS > table_words)
        return;
    const int ri = d[J_RI], left = d[J_NBLK] - b0;
    const int nb = max(ri > 0 ? min(ri, left) : left, 0);
    int end = (int)min(((long long)j + 1) * S, (long long)nbits);
    const uint8_t* seg = streams + soff;
    int16_t* out = coef + ((long long)d[J_COEF] + b0) * 64;
    int p = (int)((unsigned)sy.x >> 6), nby = nbytes, nbi = nbits;
    const int k = sy.x & 63;
    const long long base = (long long)j * (S >> 3);               // the subsequence's first byte within the segment
    if (S <= STORE_STAGE_BITS && (S & 31) == 0 && base <= nbytes && p >= base * 8) {
        unsigned* mine = stage + tid * STORE_STAGE_WORDS;
        const uint8_t* src = seg + base;
        const int have = min(nbytes - (int)base, STORE_STAGE_WORDS * 4);
#pragma unroll
        for (int i = 0; i < STORE_STAGE_WORDS; ++i) {
            unsigned v = 0;
            if (4 * i + 4 <= have) {
                __builtin_memcpy(&v, src + 4 * i, 4);              // the stream's alignment is arbitrary
            } else {
                for (int c = 0; c < 4; ++c)
                    if (4 * i + c < have) v |= (unsigned)src[4 * i + c] << (8 * c);
            }
            mine[i] = v;
        }
        seg = reinterpret_cast<const uint8_t*>(mine);
        p -= (int)base * 8;
        end -= (int)base * 8;
        nby -= (int)base;
        nbi -= (int)base * 8;
    }
    if (ok0 && dc == dc0 && ac == ac0)
        span<true>(seg, nby, nbi, tab[0], tab[1], p, k, end, out, sy.y, sy.z, nb, zz);
    else
        span<true>(seg, nby, nbi, tables + dc, tables + ac, p, k, end, out, sy.y, sy.z, nb, zz);
}

constexpr unsigned FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
                   FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
                   FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;
constexpr int CONST_BITS = 13, PASS1_BITS = 2;

// One pass of jpeg_idct_islow over eight values, on wrapping 32-bit words.  FIRST: the column pass, descaled by CONST_BITS -
// PASS1_BITS with rounding.  Otherwise the row pass: the fudge 1 << (PASS1_BITS + 2) goes to the DC term, which carries it as
// 1 << 17 into all eight sums, and the descale by CONST_BITS + PASS1_BITS + 3 rounds no further.
template <bool FIRST>
MTMP_DEV void islow_pass(const unsigned (&x)[8], int (&y)[8]) {
    unsigned z2 = x[2], z3 = x[6];
    unsigned z1 = (z2 + z3) * FIX_0_541196100;
    unsigned tmp2 = z1 - z3 * FIX_1_847759065;
    unsigned tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = FIRST ? x[0] : x[0] + (1u << (PASS1_BITS + 2));
    z3 = x[4];
    unsigned tmp0 = (z2 + z3) << CONST_BITS, tmp1 = (z2 - z3) << CONST_BITS;
    const unsigned tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7];
    tmp1 = x[5];
    tmp2 = x[3];
    tmp3 = x[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    unsigned z4 = tmp1 + tmp3;
    const unsigned z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 *= FIX_0_298631336;
    tmp1 *= FIX_2_053119869;
    tmp2 *= FIX_3_072711026;
    tmp3 *= FIX_1_501321110;
    z1 = 0u - z1 * FIX_0_899976223;
    z2 = 0u - z2 * FIX_2_562915447;
    z3 = z5 - z3 * FIX_1_961570560;
    z4 = z5 - z4 * FIX_0_390180644;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const unsigned o[8] = {tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                           tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3};
#pragma unroll
    for (int i = 0; i < 8; ++i)
        y[i] = FIRST ? (int)(o[i] + (1u << (CONST_BITS - PASS1_BITS - 1))) >> (CONST_BITS - PASS1_BITS)
                     : (int)o[i] >> (CONST_BITS + PASS1_BITS + 3);
}

// libjpeg's sample_range_limit table as jpeg_idct_islow reads it, range_limit[x & RANGE_MASK] behind the table's centre
// (jdmaster.c prepare_range_limit_table): 0..127 -> 128 + x, 128..511 -> 255, 512..895 -> 0, 896..1023 -> x - 896.  For every
// x in [-512, 511] that is clamp(x + 128, 0, 255); beyond that the table wraps, and so does this.
MTMP_DEV unsigned range_limit(int x) {
    const unsigned v = (unsigned)x & 1023u;
    return v < 128u ? v + 128u : v < 512u ? 255u : v < 896u ? 0u : v - 896u;
}

constexpr int IDCT_BLOCKS = 32;                    // 8 x 8 blocks per workgroup of 256 lanes

// Grid (groups of IDCT_BLOCKS blocks, images).  Rows >= h and columns >= w of the last blocks are dropped; an image whose status
// word is set is written as zeros.  Single byte stores: the destination offset and the row stride w are arbitrary.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const int* __restrict__ desc,
                                                        const int* __restrict__ tables, const int* __restrict__ status,
                                                        uint8_t* __restrict__ pixels) {
    __shared__ int ws[IDCT_BLOCKS][8][9];
    const int tid = threadIdx.x, img = blockIdx.y, sub = tid >> 3, lane = tid & 7;
    const int* d = desc + (long long)img * JPG_WORDS;
    const int nblk = d[J_NBLK], blk = blockIdx.x * IDCT_BLOCKS + sub;
    if (blockIdx.x * IDCT_BLOCKS >= nblk) return;  // uniform: the grid is sized for the largest image of the batch
    const bool live = blk < nblk, bad = status[img] != 0;
    if (live && !bad) {
        const int16_t* c = coef + ((long long)d[J_COEF] + blk) * 64 + lane;
        const int* q = tables + d[J_QT] + lane;
        unsigned x[8];
        int y[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = (unsigned)((int)c[r * 8] * q[r * 8]);
        islow_pass<true>(x, y);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[sub][r][lane] = y[r];
    }
    __syncthreads();
    if (!live) return;
    const int h = d[J_H], w = d[J_W], bpr = d[J_BPR];
    const int yy = (blk / bpr) * 8 + lane, x0 = (blk % bpr) * 8;
    if (yy >= h) return;
    int y[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!bad) {
        unsigned x[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = (unsigned)ws[sub][lane][c];
        islow_pass<false>(x, y);
    }
    uint8_t* dst = pixels + d[J_DST] + (long long)yy * w + x0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (x0 + c < w) dst[c] = bad ? (uint8_t)0 : (uint8_t)range_limit(y[c]);
}

}  // namespace

extern "C" int mtmp_jpeg_entropy(const uint8_t* streams, const int32_t* desc, const int32_t* segs, const int32_t* tables,
                                 int16_t* coef, int32_t* status, int32_t* rounds, int n_seg, int max_seg_bytes, int subseq_bits,
                                 int stage_bytes, void* stream) {
    MTMP_CHECK_ARG(streams && desc && segs && tables && coef && status && n_seg > 0 && max_seg_bytes >= 0 &&
                       max_seg_bytes <= MAX_SEGMENT_BYTES && subseq_bits >= 0 && stage_bytes >= 0 &&
                       stage_bytes <= MAX_STAGE_BYTES,
                   "mtmp_jpeg_entropy: bad argument (n_seg=%d max_seg_bytes=%d subseq_bits=%d stage_bytes=%d)", n_seg, max_seg_bytes,
                   subseq_bits, stage_bytes);
    const long long lanes = subseq_bits ? ((long long)max_seg_bytes * 8 + subseq_bits - 1) / subseq_bits : 1;
    MTMP_CHECK_ARG(lanes <= MAX_SUBSEQ, "mtmp_jpeg_entropy: a segment of %d bytes has %lld subsequences of %d bits (limit %d)",
                   max_seg_bytes, lanes, subseq_bits, MAX_SUBSEQ);
    const int threads = (int)((lanes < 1 ? 1 : lanes) + 63) / 64 * 64;
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3(n_seg), dim3(threads), (size_t)stage_bytes, (hipStream_t)stream, streams, desc,
                       segs, tables, coef, status, rounds, subseq_bits, stage_bytes, (const int*)nullptr, (int4*)nullptr, 0ll);
    MTMP_CHECK_LAUNCH("mtmp_jpeg_entropy");
    return MTMP_OK;
}

extern "C" int mtmp_jpeg_sync_points(const uint8_t* streams, const int32_t* desc, const int32_t* segs, const int32_t* tables,
                                     const int32_t* sync0, int32_t* sync, int32_t* status, int n_seg, int max_lanes,
                                     long long n_sync, int stage_bytes, void* stream) {
    MTMP_CHECK_ARG(streams && desc && segs && tables && sync0 && sync && status && n_seg > 0 && max_lanes > 0 &&
                       max_lanes <= MAX_SUBSEQ && n_sync > 0 && stage_bytes >= 0 && stage_bytes <= MAX_STAGE_BYTES &&
                       ((uintptr_t)sync & 15) == 0,
                   "mtmp_jpeg_sync_points: bad argument (n_seg=%d max_lanes=%d n_sync=%lld stage_bytes=%d)", n_seg, max_lanes, n_sync,
                   stage_bytes);
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3(n_seg), dim3((max_lanes + 63) / 64 * 64), (size_t)stage_bytes,
                       (hipStream_t)stream, streams, desc, segs, tables, (int16_t*)nullptr, status, (int*)nullptr, 0, stage_bytes, sync0,
                       (int4*)sync, n_sync);
    MTMP_CHECK_LAUNCH("mtmp_jpeg_sync_points");
    return MTMP_OK;
}

extern "C" int mtmp_jpeg_store_entropy(const uint8_t* streams, const int32_t* segs, const int32_t* sync, const int32_t* tables,
                                       const int32_t* desc, const long long* wide, const int32_t* prefix, int16_t* coef, int n,
                                       int total_lanes, long long stream_bytes, long long n_segs, long long n_sync,
                                       long long table_words, void* stream) {
    MTMP_CHECK_ARG(streams && segs && sync && tables && desc && wide && prefix && coef && n > 0 && total_lanes > 0 &&
                       stream_bytes > 0 && n_segs > 0 && n_sync > 0 && table_words > 0 && ((uintptr_t)sync & 15) == 0 &&
                       ((uintptr_t)wide & 7) == 0,
                   "mtmp_jpeg_store_entropy: bad argument (n=%d total_lanes=%d stream_bytes=%lld n_segs=%lld n_sync=%lld)", n,
                   total_lanes, stream_bytes, n_segs, n_sync);
    hipLaunchKernelGGL(jpeg_store_entropy_kernel, dim3((total_lanes + STORE_LANES - 1) / STORE_LANES), dim3(STORE_LANES), 0,
                       (hipStream_t)stream, streams, segs, (const int4*)sync, tables, desc, wide, prefix, coef, n, total_lanes,
                       stream_bytes, n_segs, n_sync, table_words);
    MTMP_CHECK_LAUNCH("mtmp_jpeg_store_entropy");
    return MTMP_OK;
}

extern "C" int mtmp_jpeg_idct(const int16_t* coef, const int32_t* desc, const int32_t* tables, const int32_t* status,
                              uint8_t* pixels, int n, int max_blocks, void* stream) {
    MTMP_CHECK_ARG(coef && desc && tables && status && pixels && n > 0 && n <= 65535 && max_blocks > 0,
                   "mtmp_jpeg_idct: bad argument (n=%d max_blocks=%d)", n, max_blocks);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS, n), dim3(256), 0, (hipStream_t)stream,
                       coef, desc, tables, status, pixels);
    MTMP_CHECK_LAUNCH("mtmp_jpeg_idct");
    return MTMP_OK;
}
