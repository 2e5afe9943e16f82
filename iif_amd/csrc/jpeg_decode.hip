// Baseline JPEG decoding for gfx950 (MI355X): iif_jpeg_decode (include/iif_amd.h) turns the entropy-coded scans the workers
// packed (iif_amd/jpeg.py: one record per image, its table block, its scan bytes) into the uint8 HWC regions iif_lt_augment
// reads, equal byte for byte to libjpeg's default decode (PIL's Image.open(f).convert("RGB")).  Two launches:
//
// jpeg_scan_kernel, one 256-thread workgroup per image:
//   1. destuff: the first marker that is neither stuffing (FF 00), fill (FF FF) nor RSTn ends the scan; the bytes before
//      it are compacted (FF 00 -> FF, markers dropped) into the scratch by a block-wide scan, and every RSTn records where
//      its restart interval starts;
//   2. entropy decoding, parallel within the image:
//      - with restart intervals: one thread per interval, from the interval of the box's first MCU to that of its last
//        (DC predictions start at 0 in each).  An interval is not split further, so a file with few long intervals is
//        decoded by few threads (profiles/jpeg_input_rates.txt measures one restart per MCU row);
//      - without: the scan is cut into subsequences of `subseq_bits` bits.  Each is decoded speculatively from its first
//        bit as if a block started there; then, round after round, every subsequence whose start state (bit offset, block
//        in the MCU, coefficient index) differs from its predecessor's end state is decoded again from that state, until
//        no start changes (self-synchronisation, Weissenberger & Schmidt: Huffman codes resynchronise within a few hundred
//        bits, so a few rounds do; an invalid code met while guessing only means the guess was wrong, and decoding guesses
//        again one bit further).  After kMaxRounds rounds one thread walks the rest of the chain, so a scan that never
//        synchronises costs at most kMaxRounds parallel rounds plus one serial decode, and is still exact.  Scans of the per-subsequence block counts
//        and DC difference sums give each subsequence its first block index and DC predictions; a last pass writes the
//        coefficients of the blocks inside the box's MCU window and stops after the box's last MCU;
//   3. dequantisation and libjpeg's ISLOW IDCT (jidctint.c with its range limit) of the window's blocks, one uint8 plane
//      per component.
// jpeg_pixel_kernel: per output pixel, the chroma upsampled as libjpeg's defaults do (jdsample.c h2v1 / h2v2 "fancy"
//   triangle filters with their rounding biases, edge samples replicated; plain replication when the chroma plane is at
//   most 2 samples wide), YCbCr -> RGB in jdcolor's 16-bit fixed point, grey repeated, stored HWC.
//
// tests/jpeg_ref.py restates every stage in numpy.
//
// Robustness: each record is checked against the buffers it points into before anything is read (a bad record reads
// nothing; its region is filled when the record's region offset and size are in bounds); the bit reader returns zeros past the destuffed bytes; an invalid code, a coefficient index
// past 63, a scan that ends before the box's last MCU or a missing restart marker stops that image, whose region is then
// filled with IIF_JPEG_FILL and whose status word names the reason.  The other images of the batch are unaffected.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / IIF_WAVE;
constexpr int kPixThreads = 256;
constexpr int kPixBlocks = 32;          // pixel-kernel workgroups per image
constexpr int kHuffBytes = 1424;        // look uint16 [512], maxcode int32 [18], valoff int32 [18], vals uint8 [256]
constexpr int kSlots = 6;
constexpr int kTableBytes = 3 * 64 * 2 + kSlots * kHuffBytes;
constexpr int kSubWords = 20;           // per subsequence: start (p, u, z), two end states of 8 words
constexpr int kEndA = 3, kEndB = 11;
constexpr int kMaxRounds = 8;           // synchronisation rounds before the serial fallback
enum { R_SCAN, R_SCAN_LEN, R_TABLES, R_H, R_W, R_NCOMP, R_HMAX, R_VMAX, R_DRI, R_TOP, R_LEFT, R_BH, R_BW, R_OUT, R_SCRATCH,
       R_SCRATCH_LEN, R_COMP0 };
enum { E_P, E_U, E_Z, E_NB, E_DC0, E_DC1, E_DC2, E_ERR };      // end-state words

__constant__ unsigned char kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                           12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                           58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegArgs {
    const unsigned char* data; int64_t data_bytes;
    const int64_t* rec; int n;
    unsigned char* scratch; int64_t scratch_bytes;
    unsigned char* out; int64_t out_bytes;
    int sbits;
    int* status;
};

// one image's geometry, derived from its record (iif_amd/jpeg.py window / scratch_bytes restate it)
struct Geo {
    int ok, fill;                                       // decodable; or at least the region can be filled
    int h, w, ncomp, hmax, vmax, dri, top, left, bh, bw;
    int mcux, bpm, my0, my1, mx0, mx1, need, nint, nblk;
    int ucomp[6], uby[6], ubx[6];                       // per block of an MCU: component, block row / column in it
    int ch[3], cv[3], cbw[3], cblk0[3], dcs[3], acs[3];  // per component: factors, plane blocks per row, first block, slots
    int64_t scan, scan_len, tables, out, scratch;
    int64_t o_seg, o_state, o_coef, o_plane[3];
};

__device__ __forceinline__ int64_t al16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// Record -> geometry with every check; thread 0 only.
__device__ void setup(const JpegArgs& a, int img, Geo& g) {
    g.ok = g.fill = 0;
    int64_t v[R_COMP0 + 3];
    const int64_t* r = a.rec + (int64_t)img * IIF_JPEG_REC_WORDS;
    for (int k = 0; k < R_COMP0 + 3; ++k) v[k] = r[k];
    if (v[R_BH] >= 1 && v[R_BH] <= 65535 && v[R_BW] >= 1 && v[R_BW] <= 65535 && v[R_OUT] >= 0 &&
        v[R_OUT] <= a.out_bytes - v[R_BH] * v[R_BW] * 3) {          // a bad record whose region is in bounds is filled
        g.fill = 1;
        g.bh = (int)v[R_BH]; g.bw = (int)v[R_BW]; g.out = v[R_OUT];
    }
    const int64_t H = v[R_H], W = v[R_W], nc = v[R_NCOMP];
    if (H < 1 || H > 65535 || W < 1 || W > 65535 || (nc != 1 && nc != 3)) return;
    const int64_t hm = nc == 3 ? v[R_HMAX] : 1, vm = nc == 3 ? v[R_VMAX] : 1;
    if (hm < 1 || hm > 2 || vm < 1 || vm > hm || v[R_DRI] < 0 || v[R_DRI] > 65535) return;
    const int64_t top = v[R_TOP], left = v[R_LEFT], bh = v[R_BH], bw = v[R_BW];
    if (top < 0 || left < 0 || bh < 1 || bw < 1 || top + bh > H || left + bw > W) return;
    const int64_t scan = v[R_SCAN], len = v[R_SCAN_LEN], tab = v[R_TABLES];
    if (scan < 0 || (scan & 15) || len < 0 || len > (1 << 27) || scan > a.data_bytes - len) return;
    if (tab < 0 || (tab & 15) || tab > a.data_bytes - kTableBytes) return;
    if (v[R_OUT] < 0 || v[R_OUT] > a.out_bytes - bh * bw * 3) return;
    const int64_t so = v[R_SCRATCH], sl = v[R_SCRATCH_LEN];
    if (so < 0 || (so & 15) || sl < 0 || so > a.scratch_bytes - sl) return;
    g.h = (int)H; g.w = (int)W; g.ncomp = (int)nc; g.hmax = (int)hm; g.vmax = (int)vm; g.dri = (int)v[R_DRI];
    g.top = (int)top; g.left = (int)left; g.bh = (int)bh; g.bw = (int)bw;
    const int mh = 8 * g.vmax, mw = 8 * g.hmax;
    g.mcux = (g.w + mw - 1) / mw;
    const int y0 = g.top, y1 = g.top + g.bh - 1, x0 = g.left, x1 = g.left + g.bw - 1;
    int my0 = y0 / mh, my1 = y1 / mh, mx0 = x0 / mw, mx1 = x1 / mw;
    if (g.ncomp == 3 && g.vmax == 2) {
        const int dh = (g.h + 1) / 2;
        my0 = min(my0, max(0, y0 / 2 - 1) / 8);
        my1 = max(my1, min(dh - 1, y1 / 2 + 1) / 8);
    }
    if (g.ncomp == 3 && g.hmax == 2) {
        const int dw = (g.w + 1) / 2;
        mx0 = min(mx0, max(0, x0 / 2 - 1) / 8);
        mx1 = max(mx1, min(dw - 1, x1 / 2 + 1) / 8);
    }
    g.my0 = my0; g.my1 = my1 + 1; g.mx0 = mx0; g.mx1 = mx1 + 1;
    g.need = (g.my1 - 1) * g.mcux + g.mx1;
    g.nint = g.dri ? (g.need + g.dri - 1) / g.dri : 0;
    const int64_t nsub_cap = g.dri ? 0 : max((int64_t)1, (len * 8 + a.sbits - 1) / a.sbits);
    g.bpm = 0;
    g.nblk = 0;
    int cn[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        g.cblk0[c] = g.nblk;
        g.dcs[c] = g.acs[c] = 0;
        if (c >= g.ncomp) continue;
        const int64_t cw = v[R_COMP0 + c];
        g.dcs[c] = (int)(cw & 15);
        g.acs[c] = (int)((cw >> 4) & 15);
        if (g.dcs[c] >= kSlots || g.acs[c] >= kSlots) return;
        g.ch[c] = c == 0 ? g.hmax : 1;
        g.cv[c] = c == 0 ? g.vmax : 1;
        for (int by = 0; by < g.cv[c]; ++by)
            for (int bx = 0; bx < g.ch[c]; ++bx) {
                g.ucomp[g.bpm] = c; g.uby[g.bpm] = by; g.ubx[g.bpm] = bx;
                ++g.bpm;
            }
        g.cbw[c] = (g.mx1 - g.mx0) * g.ch[c];
        cn[c] = g.cbw[c] * (g.my1 - g.my0) * g.cv[c];
        g.nblk += cn[c];
    }
    int64_t o = al16(len + 16);
    g.o_seg = o;   o += al16(4 * (int64_t)(g.nint + 1));
    g.o_state = o; o += al16(4 * (int64_t)kSubWords * nsub_cap);
    g.o_coef = o;  o += al16(128 * (int64_t)g.nblk);
    for (int c = 0; c < g.ncomp; ++c) {
        g.o_plane[c] = o;
        o += al16(64 * (int64_t)cn[c]);
    }
    if (o > sl) return;
    g.scan = scan; g.scan_len = len; g.tables = tab; g.out = v[R_OUT]; g.scratch = so;
    g.ok = 1;
}

__device__ unsigned block_excl_scan(unsigned v, unsigned* red, unsigned& total) {
    const int lane = threadIdx.x & (IIF_WAVE - 1), wv = threadIdx.x / IIF_WAVE;
    unsigned x = v;
#pragma unroll
    for (int o = 1; o < IIF_WAVE; o <<= 1) {
        const unsigned y = __shfl_up(x, o, IIF_WAVE);
        if (lane >= o) x += y;
    }
    if (lane == IIF_WAVE - 1) red[wv] = x;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const unsigned r = red[k];
        off += k < wv ? r : 0u;
        tot += r;
    }
    __syncthreads();
    total = tot;
    return off + x - v;
}

// 16 scan bytes from i0 (and the one after them) into b[0..16]; zeros past n (the readable bytes from src)
__device__ __forceinline__ void load17(const unsigned char* src, int i0, int n, int64_t avail, unsigned char (&b)[17]) {
    if ((int64_t)i0 + 16 <= avail) {
        const uint4 q = *(const uint4*)(src + i0);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) b[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (i0 + j >= n) b[j] = 0;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) b[j] = i0 + j < n ? src[i0 + j] : 0;
    }
    b[16] = i0 + 16 < n ? src[i0 + 16] : 0;
}

__device__ __forceinline__ bool is_rst(int x) { return x >= 0xD0 && x <= 0xD7; }

// MSB-first reader over the destuffed bytes (big-endian words; zeros past nw words)
struct Reader {
    const unsigned* w; int nw; int ck; uint64_t x;
    __device__ __forceinline__ unsigned ld(int k) const { return k < nw ? __builtin_bswap32(w[k]) : 0u; }
    __device__ __forceinline__ unsigned peek(int p) {
        const int k = p >> 5;
        if (k != ck) {
            x = k == ck + 1 ? (x << 32) | ld(k + 1) : ((uint64_t)ld(k) << 32) | ld(k + 1);
            ck = k;
        }
        return (unsigned)((x << (p & 31)) >> 32);
    }
};

struct Dec { int p, u, z, nb, err, dc0, dc1, dc2; };      // DC sums / predictions per component

struct Ctx {
    const unsigned* bits; int nw;
    const unsigned char* huff;      // LDS
    const unsigned char* nat;       // LDS
    const Geo* g;                   // LDS
    short* coef;
};

// the coefficient block of global block index b, or nullptr outside the box's MCU window
__device__ __forceinline__ short* locate(const Geo& g, short* coef, int64_t b) {
    const unsigned m = (unsigned)b / (unsigned)g.bpm, u = (unsigned)b - m * (unsigned)g.bpm;    // < 2^31 blocks (setup)
    const int my = (int)(m / (unsigned)g.mcux), mx = (int)(m - (unsigned)my * (unsigned)g.mcux);
    if (my < g.my0 || my >= g.my1 || mx < g.mx0 || mx >= g.mx1) return nullptr;
    const int c = g.ucomp[u];
    const int row = (my - g.my0) * g.cv[c] + g.uby[u], col = (mx - g.mx0) * g.ch[c] + g.ubx[u];
    return coef + ((int64_t)g.cblk0[c] + (int64_t)row * g.cbw[c] + col) * 64;
}

// Decode codewords while the bit offset is below `limit` (and, writing, until block `bneed`); a codeword that ends past
// `hard` is a truncated scan.  Without kWrite it only advances the state and sums block counts / DC differences: that is
// speculation, and an invalid code there only means the guessed state was wrong, so the decoder guesses again one bit
// further (a correct start never meets one in a valid stream; the writing pass, which starts from the synchronised state,
// reports it).  With kWrite d.dc holds the running DC predictions and the coefficients of window blocks are stored.
// Returns the block index.
template <bool kWrite>
__device__ int64_t run(const Ctx& x, Dec& d, int limit, int hard, int64_t b, int64_t bneed) {
    const Geo& g = *x.g;
    Reader rd{x.bits, x.nw, -2, 0};
    short* blk = kWrite && b < bneed ? locate(g, x.coef, b) : nullptr;
    // in registers: the component of block u of an MCU is arithmetic, its tables are one of three
    const int bpm = g.bpm, hv = g.ncomp == 3 ? g.hmax * g.vmax : 1;
    const unsigned char* tdc0 = x.huff + g.dcs[0] * kHuffBytes, *tdc1 = x.huff + g.dcs[1] * kHuffBytes;
    const unsigned char* tdc2 = x.huff + g.dcs[2] * kHuffBytes, *tac0 = x.huff + g.acs[0] * kHuffBytes;
    const unsigned char* tac1 = x.huff + g.acs[1] * kHuffBytes, *tac2 = x.huff + g.acs[2] * kHuffBytes;
// an error: speculation guesses again one bit further, the writing pass stops
#define IIF_JPEG_FAIL(code)     \
    {                           \
        if (!kWrite) {          \
            ++d.p;              \
            d.u = d.z = 0;      \
            continue;           \
        }                       \
        d.err = (code);         \
        break;                  \
    }
    while (d.p < limit) {
        if (kWrite && b >= bneed) break;
        const int c = d.u < hv ? 0 : d.u - hv + 1;
        const unsigned char* t = d.z == 0 ? (c == 0 ? tdc0 : c == 1 ? tdc1 : tdc2) : (c == 0 ? tac0 : c == 1 ? tac1 : tac2);
        const unsigned w = rd.peek(d.p);
        int len, sym;
        const unsigned e = ((const unsigned short*)t)[w >> 23];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255);
        } else {
            const int* maxcode = (const int*)(t + 1024);
            len = 10;
            int code = (int)(w >> 22);
            while (len <= 16 && code > maxcode[len]) {
                ++len;
                code = (int)(w >> (32 - len));
            }
            if (len > 16) IIF_JPEG_FAIL(IIF_JPEG_BAD_CODE)
            sym = t[1168 + ((((const int*)(t + 1096))[len] + code) & 255)];
        }
        const int s = sym & 15, r = sym >> 4;
        if (d.z == 0 && r) IIF_JPEG_FAIL(IIF_JPEG_BAD_CODE)         // a DC category above 15
        int v = 0;
        if (s) {
            const unsigned bits = (w << len) >> (32 - s);
            v = bits < (1u << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits;
        }
        d.p += len + s;
        if (d.p > hard) { d.err = IIF_JPEG_TRUNCATED; break; }
        if (d.z == 0) {
            const int dc = (c == 0 ? d.dc0 : c == 1 ? d.dc1 : d.dc2) + v;
            if (c == 0) d.dc0 = dc;
            else if (c == 1) d.dc1 = dc;
            else d.dc2 = dc;
            if (kWrite && blk) blk[0] = (short)dc;
            d.z = 1;
        } else if (s) {
            d.z += r;
            if (d.z > 63) IIF_JPEG_FAIL(IIF_JPEG_OVERFLOW)
            if (kWrite && blk) blk[x.nat[d.z]] = (short)v;
            ++d.z;
        } else if (r == 15) {
            d.z += 16;
            if (d.z > 64) IIF_JPEG_FAIL(IIF_JPEG_OVERFLOW)
        } else {
            d.z = 64;
        }
        if (d.z == 64) {
            d.z = 0;
            ++d.nb;
            if (++d.u == bpm) d.u = 0;
            if (kWrite) {
                ++b;
                blk = b < bneed ? locate(g, x.coef, b) : nullptr;
            }
        }
    }
#undef IIF_JPEG_FAIL
    return b;
}

__device__ __forceinline__ void put_end(int* e, const Dec& d) {
    e[E_P] = d.err ? -1 : d.p; e[E_U] = d.u; e[E_Z] = d.z; e[E_NB] = d.nb;
    e[E_DC0] = d.dc0; e[E_DC1] = d.dc1; e[E_DC2] = d.dc2; e[E_ERR] = d.err;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's post-IDCT range limit of a centred value (its table indexed by the value masked to 10 bits)
__device__ __forceinline__ unsigned range_limit(int x) {
    x &= 1023;
    return x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896;
}

// jidctint.c's 1-D pass on x[0..7] (stride-free), results before the descale in the order 0..7
__device__ __forceinline__ void butterfly(const int (&x)[8], int (&o)[8]) {
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * -15137;
    int tmp3 = z1 + z2 * 6270;
    int tmp0 = (x[0] + x[4]) * 8192;
    int tmp1 = (x[0] - x[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3; o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1; o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// dequantise + jpeg_idct_islow of one block into an 8 x 8 patch of a plane (row pitch `pitch`, 8-byte aligned rows)
__device__ void idct_block(const short* cf, const short* q, unsigned char* dst, int pitch) {
    unsigned cw[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 v = ((const uint4*)cf)[k];
        cw[4 * k] = v.x; cw[4 * k + 1] = v.y; cw[4 * k + 2] = v.z; cw[4 * k + 3] = v.w;
    }
    int ws[64];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = 8 * r + col;
            x[r] = (int)(short)(cw[k >> 1] >> (16 * (k & 1))) * (int)q[k];
        }
        butterfly(x, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[8 * r + col] = descale(o[r], 11);
    }
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        int x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = ws[8 * row + k];
        butterfly(x, o);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= range_limit(descale(o[k], 18)) << (8 * k);
            hi |= range_limit(descale(o[k + 4], 18)) << (8 * k);
        }
        *(uint2*)(dst + (int64_t)row * pitch) = make_uint2(lo, hi);
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(JpegArgs a) {
    __shared__ Geo g;
    __shared__ __attribute__((aligned(16))) unsigned char huff[kSlots * kHuffBytes];
    __shared__ short qt[3 * 64];
    __shared__ unsigned char nat[64];
    __shared__ unsigned red[kWaves];
    __shared__ int s_end, s_err, s_flag;
    const int t = threadIdx.x, img = blockIdx.x;
    if (t == 0) {
        setup(a, img, g);
        s_err = 0;
    }
    if (t < 64) nat[t] = kNatural[t];
    __syncthreads();
    if (!g.ok) {
        if (t == 0) a.status[img] = IIF_JPEG_BAD_RECORD;
        return;
    }
    const unsigned char* tab = a.data + g.tables;
    for (int k = t; k < 3 * 64; k += kThreads) qt[k] = ((const short*)tab)[k];
    for (int k = t; k < kSlots * kHuffBytes / 16; k += kThreads) ((uint4*)huff)[k] = ((const uint4*)(tab + 384))[k];

    // 1. destuff
    unsigned char* sc = a.scratch + g.scratch;
    const unsigned char* src = a.data + g.scan;
    const int n = (int)g.scan_len;
    const int64_t avail = a.data_bytes - g.scan;
    if (t == 0) s_end = n;
    __syncthreads();
    for (int i0 = t * 16; i0 < n; i0 += kThreads * 16) {
        if (i0 > *(volatile int*)&s_end) break;         // an end marker was found before this chunk
        unsigned char b[17];
        load17(src, i0, n, avail, b);
        int first = n;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = i0 + j;
            const int nx = i + 1 < n ? (int)b[j + 1] : -1;
            if (i < n && b[j] == 0xFF && !(nx == 0 || nx == 0xFF || is_rst(nx))) first = min(first, i);
        }
        if (first < n) atomicMin(&s_end, first);
    }
    __syncthreads();
    const int end = s_end;
    int* seg = (int*)(sc + g.o_seg);
    unsigned base = 0, nrst = 0;
    for (int c0 = 0; c0 < end; c0 += kThreads * 16) {
        const int i0 = c0 + t * 16;
        unsigned char b[17];
        load17(src, i0, n, avail, b);
        const int pv = i0 > 0 && i0 - 1 < n ? (int)src[i0 - 1] : 0;
        unsigned keep = 0, rst = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = i0 + j, by = b[j], prev = j ? (int)b[j - 1] : pv, nx = b[j + 1];
            if (i < end) {
                if (by == 0xFF) {
                    if (nx == 0) keep |= 1u << j;
                    else if (is_rst(nx)) rst |= 1u << j;
                } else if (!(prev == 0xFF && (by == 0 || is_rst(by)))) {
                    keep |= 1u << j;
                }
            }
        }
        unsigned total;
        const unsigned ex = block_excl_scan((unsigned)__popc(keep) | ((unsigned)__popc(rst) << 20), red, total);
        unsigned pos = base + (ex & 0xFFFFFu), rk = nrst + (ex >> 20);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((rst >> j) & 1) {
                ++rk;
                if (g.dri && rk <= (unsigned)g.nint) seg[rk] = (int)pos;
            }
            if ((keep >> j) & 1) sc[pos++] = b[j];
        }
        base += total & 0xFFFFFu;
        nrst += total >> 20;
    }
    const int nd = (int)base, nseg = (int)nrst + 1;
    if (t < 16) sc[nd + t] = 0;                 // the reader's 64-bit window may reach past the data
    if (t == 0 && g.dri) seg[0] = 0;
    {
        uint4* cz = (uint4*)(sc + g.o_coef);
        for (int k = t; k < g.nblk * 8; k += kThreads) cz[k] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();

    // 2. entropy decoding
    const Ctx x{(const unsigned*)sc, ((nd + 3) >> 2) + 2, huff, nat, &g, (short*)(sc + g.o_coef)};
    const int nbits = nd * 8;
    if (g.dri) {
        const int first = (g.my0 * g.mcux + g.mx0) / g.dri;
        for (int k = first + t; k < g.nint; k += kThreads) {
            if (k >= nseg) {
                atomicMax(&s_err, IIF_JPEG_NO_RESTART);
                continue;
            }
            Dec d{seg[k] * 8, 0, 0, 0, 0, 0, 0, 0};
            const int hard = (k + 1 < nseg ? seg[k + 1] : nd) * 8;
            const int64_t b1 = (int64_t)min((k + 1) * g.dri, g.need) * g.bpm;
            const int64_t b = run<true>(x, d, INT32_MAX, hard, (int64_t)k * g.dri * g.bpm, b1);
            if (d.err) atomicMax(&s_err, d.err);
            else if (b < b1) atomicMax(&s_err, IIF_JPEG_TRUNCATED);
        }
    } else {
        const int S = a.sbits;
        const int nsub = max(1, (nbits + S - 1) / S);
        int* st = (int*)(sc + g.o_state);
        for (int i = t; i < nsub; i += kThreads) {
            int* s = st + i * kSubWords;
            Dec d{i * S, 0, 0, 0, 0, 0, 0, 0};
            run<false>(x, d, min((i + 1) * S, nbits), INT32_MAX, 0, 0);
            s[0] = i * S; s[1] = 0; s[2] = 0;
            put_end(s + kEndA, d);
        }
        __syncthreads();
        int cur = kEndA, nxt = kEndB;
        int changed = 1;
        for (int it = 0; it < kMaxRounds && changed; ++it) {
            if (t == 0) s_flag = 0;
            __syncthreads();
            for (int i = t; i < nsub; i += kThreads) {
                int* s = st + i * kSubWords;
                if (i > 0) {
                    const int* e = st + (i - 1) * kSubWords + cur;
                    const int p = e[E_P], u = e[E_U], z = e[E_Z];
                    if (p != s[0] || (p >= 0 && (u != s[1] || z != s[2]))) {
                        s[0] = p; s[1] = u; s[2] = z;
                        Dec d{p, u, z, 0, 0, 0, 0, 0};
                        if (p < 0) d.err = IIF_JPEG_BAD_CODE;
                        else run<false>(x, d, min((i + 1) * S, nbits), INT32_MAX, 0, 0);
                        put_end(s + nxt, d);
                        s_flag = 1;
                        continue;
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) s[nxt + k] = s[cur + k];
            }
            __syncthreads();
            changed = s_flag;
            cur ^= kEndA ^ kEndB;
            nxt ^= kEndA ^ kEndB;
            __syncthreads();
        }
        if (changed) {          // not synchronised after kMaxRounds: one thread walks the chain, at most one serial decode
            if (t == 0) {
                for (int i = 1; i < nsub; ++i) {
                    int* s = st + i * kSubWords;
                    const int* e = st + (i - 1) * kSubWords + cur;
                    const int p = e[E_P], u = e[E_U], z = e[E_Z];
                    if (p != s[0] || u != s[1] || z != s[2]) {
                        s[0] = p; s[1] = u; s[2] = z;
                        Dec d{p, u, z, 0, 0, 0, 0, 0};
                        if (p < 0) d.err = IIF_JPEG_BAD_CODE;
                        else run<false>(x, d, min((i + 1) * S, nbits), INT32_MAX, 0, 0);
                        put_end(s + cur, d);
                    }
                }
            }
            __syncthreads();
        }
        // first block index and DC predictions of each subsequence: exclusive scans, kept in its `nxt` words
        unsigned carry[4] = {0, 0, 0, 0};
        for (int c0 = 0; c0 < nsub; c0 += kThreads) {
            const int i = c0 + t;
            const int* e = st + i * kSubWords + cur;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned tot;
                const unsigned ex = block_excl_scan(i < nsub ? (unsigned)e[E_NB + q] : 0u, red, tot);
                if (i < nsub) st[i * kSubWords + nxt + q] = (int)(carry[q] + ex);
                carry[q] += tot;
            }
        }
        __syncthreads();
        const int64_t bneed = (int64_t)g.need * g.bpm;
        for (int i = t; i < nsub; i += kThreads) {
            const int* s = st + i * kSubWords;
            const int64_t b0 = (unsigned)s[nxt];
            if (b0 >= bneed) continue;
            if (s[0] < 0) {
                atomicMax(&s_err, IIF_JPEG_BAD_CODE);
                continue;
            }
            Dec d{s[0], s[1], s[2], 0, 0, s[nxt + 1], s[nxt + 2], s[nxt + 3]};
            const bool last = i == nsub - 1;
            const int64_t b = run<true>(x, d, last ? INT32_MAX : min((i + 1) * S, nbits), nbits, b0, bneed);
            if (d.err) atomicMax(&s_err, d.err);
            else if (last && b < bneed) atomicMax(&s_err, IIF_JPEG_TRUNCATED);
        }
    }
    __syncthreads();
    if (s_err) {
        if (t == 0) a.status[img] = s_err;
        return;
    }

    // 3. dequantise + IDCT into the component planes
    for (int k = t; k < g.nblk; k += kThreads) {
        const int c = (k >= g.cblk0[1]) + (k >= g.cblk0[2]);
        const int kk = k - g.cblk0[c], row = kk / g.cbw[c], col = kk - row * g.cbw[c];
        const int pitch = g.cbw[c] * 8;
        idct_block((const short*)(sc + g.o_coef) + (int64_t)k * 64, qt + 64 * c,
                   sc + g.o_plane[c] + (int64_t)row * 8 * pitch + col * 8, pitch);
    }
    if (t == 0) a.status[img] = IIF_JPEG_OK;
}

// one chroma sample of component c at image pixel (y, x), upsampled as jdsample.c does
__device__ __forceinline__ int chroma(const Geo& g, const unsigned char* sc, int c, int y, int x) {
    const unsigned char* P = sc + g.o_plane[c];
    const int pw = g.cbw[c] * 8, r0 = g.my0 * 8, c0 = g.mx0 * 8;
    auto at = [&](int i, int j) { return (int)P[(int64_t)(i - r0) * pw + (j - c0)]; };
    if (g.hmax == 1) return at(y, x);
    const int dw = (g.w + 1) >> 1, j = x >> 1, odd = x & 1;
    const bool fancy = dw > 2;
    const int jn = odd ? min(j + 1, dw - 1) : max(j - 1, 0);
    if (g.vmax == 1) {
        if (!fancy) return at(y, j);
        return (3 * at(y, j) + at(y, jn) + (odd ? 2 : 1)) >> 2;
    }
    const int i = y >> 1;
    if (!fancy) return at(i, j);
    const int dh = (g.h + 1) >> 1;
    const int in = (y & 1) ? min(i + 1, dh - 1) : max(i - 1, 0);
    const int s0 = 3 * at(i, j) + at(in, j), s1 = 3 * at(i, jn) + at(in, jn);
    return (3 * s0 + s1 + (odd ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned char clamp255(int v) { return (unsigned char)min(max(v, 0), 255); }

__global__ __launch_bounds__(kPixThreads) void jpeg_pixel_kernel(JpegArgs a) {
    __shared__ Geo g;
    const int img = blockIdx.y;
    if (threadIdx.x == 0) setup(a, img, g);
    __syncthreads();
    if (!g.ok && !g.fill) return;
    const int status = g.ok ? a.status[img] : IIF_JPEG_BAD_RECORD;
    unsigned char* dst = a.out + g.out;
    const unsigned char* sc = a.scratch + g.scratch;
    const int64_t npx = (int64_t)g.bh * g.bw;
    const int mh = 8 * g.vmax, mw = 8 * g.hmax, pw0 = g.cbw[0] * 8;
    for (int64_t p = (int64_t)blockIdx.x * kPixThreads + threadIdx.x; p < npx; p += (int64_t)gridDim.x * kPixThreads) {
        unsigned char r = IIF_JPEG_FILL, gg = IIF_JPEG_FILL, b = IIF_JPEG_FILL;
        if (status == IIF_JPEG_OK) {
            const int y = g.top + (int)(p / g.bw), x = g.left + (int)(p % g.bw);
            const int Y = sc[g.o_plane[0] + (int64_t)(y - g.my0 * mh) * pw0 + (x - g.mx0 * mw)];
            if (g.ncomp == 1) {
                r = gg = b = (unsigned char)Y;
            } else {
                const int cb = chroma(g, sc, 1, y, x) - 128, cr = chroma(g, sc, 2, y, x) - 128;
                r = clamp255(Y + ((91881 * cr + 32768) >> 16));                    // jdcolor.c: FIX(1.40200)
                gg = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));     // FIX(0.34414), FIX(0.71414)
                b = clamp255(Y + ((116130 * cb + 32768) >> 16));                   // FIX(1.77200)
            }
        }
        dst[3 * p] = r;
        dst[3 * p + 1] = gg;
        dst[3 * p + 2] = b;
    }
}

}  // namespace

extern "C" int iif_jpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* rec, int64_t n, uint8_t* scratch,
                               int64_t scratch_bytes, uint8_t* out, int64_t out_bytes, int subseq_bits, int32_t* status,
                               void* stream) {
    if (!data || !rec || !scratch || !out || !status) return IIF_EINVAL;
    if (((uintptr_t)data & 15) || ((uintptr_t)scratch & 15)) return IIF_EINVAL;
    if (data_bytes < 0 || scratch_bytes < 0 || out_bytes < 0 || n < 0 || n > 65535) return IIF_EINVAL;
    if (subseq_bits < 32 || subseq_bits > (1 << 24)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    JpegArgs a{data, data_bytes, rec, (int)n, scratch, scratch_bytes, out, out_bytes, subseq_bits, status};
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)n), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pixel_kernel, dim3(kPixBlocks, (unsigned)n), dim3(kPixThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
