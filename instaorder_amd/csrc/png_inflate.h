// DEFLATE (RFC 1951) decoder of ONE stream with zlib's acceptance rules, written once for the device kernel (csrc/png.hip)
// and for a host program that runs it under the sanitizers (tests/png_inflate_host.cpp).  No HIP header is needed: with a
// plain C++ compiler the functions are ordinary inline functions and the "wave" has one lane.
//
// One wave decodes one stream.  The symbol loop is UNIFORM: every lane reads the same compressed bits (from a window of
// the data staged in LDS a coalesced chunk at a time), looks up the same table entries (two levels: a direct table over
// the first PNG_LIT_BITS / PNG_DIST_BITS bits, canonical counts behind it; built per dynamic block, in LDS) and takes the
// same branches; what the lanes share out is the data movement.  The last 32 KiB of output live in a ring in LDS:
// literals go into the ring, a match is copied ring to ring by all lanes (lane i of a chunk reads src[i mod distance], so
// an overlapping match needs no serial loop), stored blocks come from the data in coalesced pieces, and the ring is
// flushed to memory PNG_FLUSH_BYTES at a time in 16-byte stores.  Every back-reference is an LDS access.
//
// Safety does not depend on the stream.  Data bytes are read at [0, nbytes) only; past the end the window supplies zero
// bits, the bits consumed are counted, and a symbol that used one of them fails the stream.  An iteration of the symbol
// loop consumes at least one bit, so the loop ends after at most 8 * nbytes + 64 bits; the code-length loops end at 320
// entries; output is written at [0, expected) only (the check comes before the write) and a distance never reaches past
// the bytes produced, nor, being at most 32768, past the ring.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ __forceinline__
#else
#define PNG_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_SYNC() __syncthreads()
#define PNG_UNIFORM(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define PNG_SYNC() ((void)0)
#define PNG_UNIFORM(x) ((int)(x))
#endif

#define PNG_RING_BYTES 32768    // the DEFLATE window: the largest distance
#define PNG_WIN_BYTES 1024      // compressed bytes staged at a time (a multiple of 4)
#define PNG_FLUSH_BYTES 4096    // the ring goes to memory in pieces of this size (a multiple of 16 that divides the ring)
#define PNG_LIT_BITS 10         // first-level lookup of the literal/length code
#define PNG_DIST_BITS 8         // ... and of the distance code

enum {
    PNG_STATUS_OK = 0,
    PNG_STATUS_BLOCK_TYPE = 1,  // block type 3
    PNG_STATUS_STORED_LEN = 2,  // LEN and NLEN of a stored block disagree
    PNG_STATUS_CODE_SET = 3,    // a code-length set zlib's inflate_table refuses, HLIT > 286, HDIST > 30, a bad repeat, no end-of-block code
    PNG_STATUS_SYMBOL = 4,      // bits that are no code, a literal/length symbol above 285, a distance symbol above 29
    PNG_STATUS_DISTANCE = 5,    // a distance that reaches before the first output byte
    PNG_STATUS_NO_DATA = 6,     // bits were needed past the end of the data
    PNG_STATUS_SIZE = 7,        // more or fewer bytes than expected
    PNG_STATUS_ADLER = 8,       // (csrc/png.hip) Adler-32 of the inflated bytes
    PNG_STATUS_FILTER = 9       // (csrc/png.hip) a filter byte above 4
};

struct alignas(16) PngVec16 {
    uint32_t v[4];
};

// the decoder's working memory: LDS on the device (36.8 KiB; four streams per CU), any 16-byte aligned memory on the host
struct alignas(16) PngShared {
    uint8_t ring[PNG_RING_BYTES];
    uint8_t win[PNG_WIN_BYTES];
    uint16_t lit_look[1 << PNG_LIT_BITS];    // (length << 9) | symbol of the code that starts these bits, 0: none or longer
    uint16_t dist_look[1 << PNG_DIST_BITS];
    uint16_t cl_look[128];                   // the code-length code has at most 7 bits: one level
    uint16_t lit_sym[288], dist_sym[32], cl_sym[32];     // symbols in code order
    uint16_t lit_count[16], dist_count[16], cl_count[16];// codes per length
    uint16_t offs[16];
    uint8_t lens[352];                        // [0, 19): the code-length code; [32, 32 + 316): the block's two codes
};

struct PngInflate {
    PngShared* sh;
    const uint8_t* data;    // the DEFLATE bytes
    long nbytes;
    uint8_t* dst;           // receives [0, expected), 16-byte aligned
    long expected;
    int lane, lanes;
    // the bit reader: bits [0, cnt) of buf are the next bits of the stream; pos = data bytes taken into buf so far
    uint64_t buf;
    int cnt;
    long pos, win_base;     // win holds data[win_base, win_base + PNG_WIN_BYTES), zeros past nbytes
    long out, flushed;
};

PNG_HD int png_len_base(int i) {
    constexpr uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    return t[i];
}
PNG_HD int png_len_extra(int i) { return i < 8 || i == 28 ? 0 : (i - 4) >> 2; }
PNG_HD int png_dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }
PNG_HD int png_dist_base(int i) { return i < 4 ? i + 1 : ((2 + (i & 1)) << png_dist_extra(i)) + 1; }

PNG_HD void png_load_window(PngInflate& s, long at) {
    PNG_SYNC();                                             // nobody still reads the old window
    for (int i = s.lane; i < PNG_WIN_BYTES; i += s.lanes) s.sh->win[i] = at + i < s.nbytes ? s.data[at + i] : (uint8_t)0;
    s.win_base = at;
    PNG_SYNC();
}

// at least 32 valid bits in buf (zeros past the end of the data)
PNG_HD void png_refill(PngInflate& s) {
    if (s.cnt > 32) return;
    if (s.pos - s.win_base >= PNG_WIN_BYTES) png_load_window(s, s.pos);
    // pos - win_base is a multiple of 4: the window is loaded at pos, and pos moves by whole words until a stored block
    const uint32_t w = (uint32_t)PNG_UNIFORM(*reinterpret_cast<const uint32_t*>(s.sh->win + (s.pos - s.win_base)));
    s.buf |= (uint64_t)w << s.cnt;
    s.cnt += 32;
    s.pos += 4;
}
PNG_HD int png_take(PngInflate& s, int n) {                // n <= 16, n <= cnt
    const int v = (int)(s.buf & ((1u << n) - 1u));
    s.buf >>= n;
    s.cnt -= n;
    return v;
}
PNG_HD long png_bits_used(const PngInflate& s) { return 8 * s.pos - s.cnt; }
PNG_HD bool png_overrun(const PngInflate& s) { return png_bits_used(s) > 8 * s.nbytes; }

// One symbol of a code (look over `bits` bits, canonical counts / symbols behind it); -1: the next 15 bits are no code.
PNG_HD int png_symbol(PngInflate& s, const uint16_t* look, int bits, const uint16_t* count, const uint16_t* sym) {
    const int e = PNG_UNIFORM(look[s.buf & ((1u << bits) - 1u)]);
    if (e) {
        s.buf >>= (e >> 9);
        s.cnt -= (e >> 9);
        return e & 511;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)((s.buf >> (l - 1)) & 1);
        const int c = PNG_UNIFORM(count[l]);
        if (code - c < first) {
            s.buf >>= l;
            s.cnt -= l;
            return PNG_UNIFORM(sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// Tables of one code from lens[0, n): false for a set zlib's inflate_table refuses.  kind 0: the code-length code
// (complete or refused), 1: literal/length, 2: distance (may be empty); 1 and 2 may be incomplete only as one 1-bit code.
PNG_HD bool png_build(PngInflate& s, const uint8_t* lens, int n, int kind, uint16_t* look, int bits, uint16_t* count,
                      uint16_t* sym) {
    PngShared* sh = s.sh;
    PNG_SYNC();                                             // the lengths are written, the old tables no longer read
    if (s.lane == 0) {
        for (int l = 0; l < 16; ++l) count[l] = 0;
        for (int i = 0; i < n; ++i) count[lens[i] & 15]++;
    }
    for (int i = s.lane; i < (1 << bits); i += s.lanes) look[i] = 0;
    PNG_SYNC();
    int left = 1, longest = 0;
    for (int l = 1; l <= 15; ++l) {
        const int c = PNG_UNIFORM(count[l]);
        left = (left << 1) - c;
        if (left < 0) return false;                         // over-subscribed
        if (c) longest = l;
    }
    if (longest == 0) return kind == 2;                     // no code at all: only a distance code may be empty
    if (left > 0 && (kind == 0 || longest != 1)) return false;
    if (s.lane == 0) {
        int o = 0;
        for (int l = 1; l <= 15; ++l) { sh->offs[l] = (uint16_t)o; o += count[l]; }
        for (int i = 0; i < n; ++i)
            if (lens[i] & 15) sym[sh->offs[lens[i] & 15]++] = (uint16_t)i;
    }
    PNG_SYNC();
    int code = 0, index = 0;
    for (int l = 1; l <= bits; ++l) {                        // the direct table: every lane walks the codes, the fill is shared out
        const int c = PNG_UNIFORM(count[l]);
        for (int j = 0; j < c; ++j, ++code, ++index) {
            int rev = 0;
            for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1) << (l - 1 - b);
            const uint16_t e = (uint16_t)((l << 9) | PNG_UNIFORM(sym[index]));
            for (int f = rev + (s.lane << l); f < (1 << bits); f += s.lanes << l) look[f] = e;
        }
        code <<= 1;
    }
    PNG_SYNC();
    return true;
}

PNG_HD void png_flush(PngInflate& s) {                      // one piece of the ring to memory; out - flushed >= PNG_FLUSH_BYTES
    PNG_SYNC();
    const uint8_t* src = s.sh->ring + (s.flushed & (PNG_RING_BYTES - 1));
    for (int i = 16 * s.lane; i < PNG_FLUSH_BYTES; i += 16 * s.lanes)
        *reinterpret_cast<PngVec16*>(s.dst + s.flushed + i) = *reinterpret_cast<const PngVec16*>(src + i);
    s.flushed += PNG_FLUSH_BYTES;
}

PNG_HD void png_build_fixed(PngInflate& s) {
    PngShared* sh = s.sh;
    PNG_SYNC();
    for (int i = s.lane; i < 288; i += s.lanes) sh->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = s.lane; i < 32; i += s.lanes) sh->lens[288 + i] = 5;
    png_build(s, sh->lens, 288, 1, sh->lit_look, PNG_LIT_BITS, sh->lit_count, sh->lit_sym);
    png_build(s, sh->lens + 288, 32, 2, sh->dist_look, PNG_DIST_BITS, sh->dist_count, sh->dist_sym);
}

// the code lengths of a dynamic block and its two codes; a status word
PNG_HD int png_dynamic_header(PngInflate& s) {
    PngShared* sh = s.sh;
    png_refill(s);
    const int nlen = png_take(s, 5) + 257, ndist = png_take(s, 5) + 1, ncode = png_take(s, 4) + 4;
    if (png_overrun(s)) return PNG_STATUS_NO_DATA;
    if (nlen > 286 || ndist > 30) return PNG_STATUS_CODE_SET;
    PNG_SYNC();
    if (s.lane == 0)
        for (int i = 0; i < 19; ++i) sh->lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        png_refill(s);
        const int v = png_take(s, 3);
        if (s.lane == 0) sh->lens[order[i]] = (uint8_t)v;
    }
    if (png_overrun(s)) return PNG_STATUS_NO_DATA;
    if (!png_build(s, sh->lens, 19, 0, sh->cl_look, 7, sh->cl_count, sh->cl_sym)) return PNG_STATUS_CODE_SET;
    int have = 0, last = -1;
    while (have < nlen + ndist) {                            // at most 316 entries, each iteration adds at least one
        png_refill(s);
        const int sym = png_symbol(s, sh->cl_look, 7, sh->cl_count, sh->cl_sym);   // a complete code: never -1
        if (sym < 0) return PNG_STATUS_CODE_SET;
        int rep = 1, val = sym;
        if (sym == 16) { rep = 3 + png_take(s, 2); val = last; }
        else if (sym == 17) { rep = 3 + png_take(s, 3); val = 0; }
        else if (sym == 18) { rep = 11 + png_take(s, 7); val = 0; }
        if (png_overrun(s)) return PNG_STATUS_NO_DATA;
        if (val < 0 || have + rep > nlen + ndist) return PNG_STATUS_CODE_SET;
        if (s.lane == 0)
            for (int i = 0; i < rep; ++i) sh->lens[32 + have + i] = (uint8_t)val;
        have += rep;
        last = val;
    }
    PNG_SYNC();
    if (PNG_UNIFORM(sh->lens[32 + 256]) == 0) return PNG_STATUS_CODE_SET;          // no end-of-block code
    if (!png_build(s, sh->lens + 32, nlen, 1, sh->lit_look, PNG_LIT_BITS, sh->lit_count, sh->lit_sym)) return PNG_STATUS_CODE_SET;
    if (!png_build(s, sh->lens + 32 + nlen, ndist, 2, sh->dist_look, PNG_DIST_BITS, sh->dist_count, sh->dist_sym))
        return PNG_STATUS_CODE_SET;
    return PNG_STATUS_OK;
}

// a stored block: LEN bytes from the data to the ring in pieces, flushed as they come
PNG_HD int png_stored(PngInflate& s) {
    png_take(s, s.cnt & 7);
    png_refill(s);
    const int len = png_take(s, 16), nlen = png_take(s, 16);
    if (png_overrun(s)) return PNG_STATUS_NO_DATA;
    if (len != (nlen ^ 0xffff)) return PNG_STATUS_STORED_LEN;
    s.pos -= s.cnt >> 3;                                     // whole bytes that were taken into buf go back
    s.buf = 0;
    s.cnt = 0;
    if (s.pos + len > s.nbytes) return PNG_STATUS_NO_DATA;
    if (s.out + len > s.expected) return PNG_STATUS_SIZE;
    int done = 0;
    while (done < len) {
        const int piece = len - done < PNG_FLUSH_BYTES ? len - done : PNG_FLUSH_BYTES;
        for (int i = s.lane; i < piece; i += s.lanes)
            s.sh->ring[(s.out + i) & (PNG_RING_BYTES - 1)] = s.data[s.pos + i];
        s.out += piece;
        s.pos += piece;
        done += piece;
        while (s.out - s.flushed >= PNG_FLUSH_BYTES) png_flush(s);
    }
    s.win_base = s.pos - PNG_WIN_BYTES;                      // the window is stale: the next refill loads it at pos
    return PNG_STATUS_OK;
}

// Inflates data[0, nbytes) into dst[0, expected); the status word (0: exactly `expected` bytes were produced).
PNG_HD int png_inflate(PngShared* sh, const uint8_t* data, long nbytes, uint8_t* dst, long expected, int lane, int lanes) {
    PngInflate s;
    s.sh = sh; s.data = data; s.nbytes = nbytes; s.dst = dst; s.expected = expected; s.lane = lane; s.lanes = lanes;
    s.buf = 0; s.cnt = 0; s.pos = 0; s.out = 0; s.flushed = 0;
    s.win_base = -PNG_WIN_BYTES;
    int final = 0;
    while (!final) {                                         // every block consumes at least its 3 header bits
        png_refill(s);
        final = png_take(s, 1);
        const int type = png_take(s, 2);
        if (png_overrun(s)) return PNG_STATUS_NO_DATA;
        if (type == 3) return PNG_STATUS_BLOCK_TYPE;
        if (type == 0) {
            const int rc = png_stored(s);
            if (rc) return rc;
            continue;
        }
        if (type == 1) {
            png_build_fixed(s);
        } else {
            const int rc = png_dynamic_header(s);
            if (rc) return rc;
        }
        const uint8_t* ring = sh->ring;
        for (;;) {                                           // every symbol consumes at least one bit
            png_refill(s);
            int sym = png_symbol(s, sh->lit_look, PNG_LIT_BITS, sh->lit_count, sh->lit_sym);
            if (sym < 0) return 8 * s.nbytes - png_bits_used(s) < 15 ? PNG_STATUS_NO_DATA : PNG_STATUS_SYMBOL;
            if (png_overrun(s)) return PNG_STATUS_NO_DATA;
            if (sym < 256) {
                if (s.out >= s.expected) return PNG_STATUS_SIZE;
                if (s.lane == 0) sh->ring[s.out & (PNG_RING_BYTES - 1)] = (uint8_t)sym;
                s.out++;
                if (s.out - s.flushed >= PNG_FLUSH_BYTES) png_flush(s);
                continue;
            }
            if (sym == 256) break;
            if (sym > 285) return PNG_STATUS_SYMBOL;
            sym -= 257;
            const int len = png_len_base(sym) + png_take(s, png_len_extra(sym));
            png_refill(s);
            const int ds = png_symbol(s, sh->dist_look, PNG_DIST_BITS, sh->dist_count, sh->dist_sym);
            if (ds < 0) return 8 * s.nbytes - png_bits_used(s) < 15 ? PNG_STATUS_NO_DATA : PNG_STATUS_SYMBOL;
            if (png_overrun(s)) return PNG_STATUS_NO_DATA;
            if (ds > 29) return PNG_STATUS_SYMBOL;
            const int dist = png_dist_base(ds) + png_take(s, png_dist_extra(ds));
            if (png_overrun(s)) return PNG_STATUS_NO_DATA;
            if (dist > s.out) return PNG_STATUS_DISTANCE;
            if (s.out + len > s.expected) return PNG_STATUS_SIZE;
            PNG_SYNC();                                      // the literals in front of the match are in the ring
            for (int i = s.lane; i < len; i += s.lanes) {
                const int k = dist >= len ? i : i % dist;    // an overlapping match repeats its first `dist` bytes
                sh->ring[(s.out + i) & (PNG_RING_BYTES - 1)] = ring[(s.out - dist + k) & (PNG_RING_BYTES - 1)];
            }
            PNG_SYNC();
            s.out += len;
            if (s.out - s.flushed >= PNG_FLUSH_BYTES) png_flush(s);
        }
    }
    if (s.out != s.expected) return PNG_STATUS_SIZE;
    PNG_SYNC();
    for (long i = s.flushed + s.lane; i < s.out; i += s.lanes) dst[i] = sh->ring[i & (PNG_RING_BYTES - 1)];
    return PNG_STATUS_OK;
}

// Adler-32 in pieces: over bytes p[i], i in the caller's share of [0, n), s1 += p[i], s2 += i * p[i] (64-bit sums cannot
// overflow for n < 2^32: s2 < 2^32 * 2^8 * 2^23 per share of a 256-way split, and the callers reduce modulo 65521 after
// each share); the checksum of the whole follows from the two totals.
PNG_HD uint32_t png_adler_finish(uint64_t s1, uint64_t s2, uint64_t n) {
    const uint64_t M = 65521;
    const uint64_t a = (1 + s1 % M) % M;
    // b = n + sum (n - i) p[i] = n + n s1 - s2
    const uint64_t b = (n % M + (n % M) * (s1 % M) % M + M - s2 % M) % M;
    return (uint32_t)((b << 16) | a);
}
