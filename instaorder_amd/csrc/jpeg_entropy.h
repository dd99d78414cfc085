// Baseline JPEG entropy decoder of ONE stream (ITU T.81 F.2.2), written once for the device kernel (csrc/jpeg.hip) and for
// a host program that runs it under the sanitizers (tests/jpeg_entropy_host.cpp).  No HIP header is needed: with a plain
// C++ compiler the functions are ordinary inline functions.
//
// The decoder is a FLAT loop: one iteration decodes one Huffman symbol (a DC category or an AC run/size) and advances the
// state (block, position k inside the block).  An iteration either moves k forward by at least one or finishes a block,
// so the loop runs at most 64 * n_blocks times whatever the bytes are; lanes that decode different images side by side
// stay in step symbol by symbol instead of waiting for each other's blocks.
//
// Safety does not depend on the stream: bytes are read at positions [0, nbytes) only (eight at a time), past the end (or past a marker) the
// reader supplies zero bits and counts them, and using one of those bits flags the stream; table indices are masked; a
// coefficient is stored at block * 64 + zigzag[k] with block < n_blocks and k <= 63 checked first.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

#define JPEG_LOOKUP_BITS 8      // codes of at most this many bits are decoded by one table read

enum {
    JPEG_STATUS_OK = 0,
    JPEG_STATUS_BAD_CODE = 1,   // the next bits are no code of the Huffman table
    JPEG_STATUS_BAD_RUN = 2,    // a zero run that ends past coefficient 63
    JPEG_STATUS_BAD_RESTART = 3,// RSTn expected: missing, out of order, or data left in front of it
    JPEG_STATUS_NO_DATA = 4,    // bits were needed past the end of the data (or past a marker inside it)
    JPEG_STATUS_BAD_DC = 5      // a DC category above 15
};

// derived decode table of one Huffman table (904 bytes)
struct JpegHuff {
    uint16_t look[1 << JPEG_LOOKUP_BITS];   // (length << 8) | symbol of the code that starts these 8 bits, 0: a longer code
    int32_t maxcode[17];                    // [l]: the largest code of length l, -1 where there is none ([0] unused)
    int32_t valoff[17];                     // [l]: index of the first symbol of length l minus its code
    uint8_t sym[256];
};

// counts[l - 1] = number of codes of length l (1..16), symbols in code order.  Returns false, and leaves a table that
// decodes nothing, unless the counts form a prefix code of at most 256 symbols (code + count <= 2^l at every length).
JPEG_HD bool jpeg_build_huff(const uint8_t* counts, const uint8_t* symbols, JpegHuff* h) {
    for (int i = 0; i < (1 << JPEG_LOOKUP_BITS); ++i) h->look[i] = 0;
    for (int l = 0; l <= 16; ++l) { h->maxcode[l] = -1; h->valoff[l] = 0; }
    for (int i = 0; i < 256; ++i) h->sym[i] = 0;
    int total = 0, code = 0;
    bool ok = true;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        if (total + c > 256 || code + c > (1 << l)) ok = false;
        if (ok) { total += c; code = (code + c) << 1; }
    }
    if (!ok) return false;
    int k = 0;
    code = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        h->valoff[l] = k - code;
        for (int j = 0; j < c; ++j) {
            const int s = symbols[k];
            h->sym[k] = (uint8_t)s;
            if (l <= JPEG_LOOKUP_BITS) {
                const int sh = JPEG_LOOKUP_BITS - l;
                for (int f = 0; f < (1 << sh); ++f) h->look[((code << sh) | f) & 255] = (uint16_t)((l << 8) | s);
            }
            ++k;
            ++code;
        }
        if (c) h->maxcode[l] = code - 1;
        code <<= 1;
    }
    return true;
}

JPEG_HD int jpeg_zigzag(int k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

// ---- bit reader: removes FF 00 stuffing, skips FF fill bytes, stops at a marker ----------------------------------------
struct JpegBits {
    const uint8_t* p;
    int32_t pos, end;
    uint64_t acc;       // the low n bits are the unread bits, oldest on top
    int32_t n;          // bits in acc
    int32_t pad;        // how many of them (the youngest) are zeros supplied past the end or past a marker
    int32_t marker;     // p[pos] = FF of a marker (or a lone FF at the end): nothing is read until a restart takes it
    int32_t overrun;    // a supplied zero bit was used
    uint64_t cache;     // the bytes p[cache_pos .. cache_pos + 8), first byte lowest (zero past the end)
    int32_t cache_pos;
};

// p[at] for 0 <= at < end.  The data is fetched eight bytes at a time (one load where eight bytes are left, single bytes
// at the tail, never a byte at or past `end`), so that most symbols need no memory read at all.
JPEG_HD uint32_t jpeg_byte(JpegBits& b, int32_t at) {
    uint32_t d = (uint32_t)(at - b.cache_pos);
    if (d >= 8u) {
        uint64_t w = 0;
        if (at + 8 <= b.end) {
            memcpy(&w, b.p + at, 8);                 // little-endian host and device
        } else {
            for (int i = 0; i < 8 && at + i < b.end; ++i) w |= (uint64_t)b.p[at + i] << (8 * i);
        }
        b.cache = w;
        b.cache_pos = at;
        d = 0;
    }
    return (uint32_t)(b.cache >> (8 * d)) & 255u;
}

// At least 32 bits afterwards: a symbol takes at most 16 + 15.  Four bytes at once where eight are left and none of the
// four is FF (no stuffing, no marker); otherwise byte by byte, every pass adding a byte to acc (at most 4 passes) or
// skipping one fill byte.
JPEG_HD void jpeg_refill(JpegBits& b) {
    if (b.n >= 32) return;
    if (!b.marker && b.pos + 8 <= b.end) {
        uint32_t d = (uint32_t)(b.pos - b.cache_pos);
        if (d > 4u) {
            memcpy(&b.cache, b.p + b.pos, 8);
            b.cache_pos = b.pos;
            d = 0;
        }
        const uint32_t w = (uint32_t)(b.cache >> (8 * d)), x = ~w;
        if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {       // no byte of w is FF
            b.acc = (b.acc << 32) | __builtin_bswap32(w);
            b.n += 32;
            b.pos += 4;
            return;
        }
    }
    while (b.n < 32) {
        uint32_t byte = 0;
        bool real = false;
        if (!b.marker && b.pos < b.end) {
            byte = jpeg_byte(b, b.pos);
            if (byte != 0xFF) {
                b.pos += 1;
                real = true;
            } else {
                const uint32_t next = b.pos + 1 < b.end ? jpeg_byte(b, b.pos + 1) : 0x100u;
                if (next == 0) {
                    b.pos += 2;
                    real = true;
                } else if (next == 0xFF) {
                    b.pos += 1;                      // a fill byte in front of a marker
                    continue;
                } else {
                    b.marker = 1;
                    byte = 0;
                }
            }
        }
        if (!real) b.pad += 8;
        b.acc = (b.acc << 8) | byte;
        b.n += 8;
    }
}

JPEG_HD uint32_t jpeg_peek(const JpegBits& b, int k) {          // 1 <= k <= 16 <= n
    return (uint32_t)(b.acc >> (b.n - k)) & ((1u << k) - 1u);
}

JPEG_HD void jpeg_skip(JpegBits& b, int k) {
    b.n -= k;
    if (b.n < b.pad) { b.overrun = 1; b.pad = b.n; }
}

// next Huffman symbol, or -1 if the bits are no code of the table; needs n >= 16
JPEG_HD int jpeg_symbol(JpegBits& b, const JpegHuff* h) {
    const uint32_t c16 = jpeg_peek(b, 16);
    const uint32_t e = h->look[c16 >> (16 - JPEG_LOOKUP_BITS)];
    if (e) {
        jpeg_skip(b, (int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = JPEG_LOOKUP_BITS + 1; l <= 16; ++l) {
        const int c = (int)(c16 >> (16 - l));
        if (c <= h->maxcode[l]) {
            jpeg_skip(b, l);
            return h->sym[(h->valoff[l] + c) & 255];
        }
    }
    return -1;
}

// the s-bit field that follows a symbol, sign-extended by T.81 F.2.2.1 (EXTEND); 1 <= s <= 15
JPEG_HD int jpeg_receive_extend(JpegBits& b, int s) {
    const int v = (int)jpeg_peek(b, s);
    jpeg_skip(b, s);
    return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
}

// the marker RST(index & 7) must be the next thing in the data, with less than one byte of real bits left in front of it
JPEG_HD bool jpeg_take_restart(JpegBits& b, int index) {
    jpeg_refill(b);
    if (!b.marker || b.n - b.pad >= 8 || b.pos + 1 >= b.end) return false;
    if (jpeg_byte(b, b.pos + 1) != (uint32_t)(0xD0 + (index & 7))) return false;
    b.pos += 2;
    b.acc = 0;
    b.n = b.pad = b.marker = 0;
    return true;
}

struct JpegScan {
    const uint8_t* data;        // the entropy-coded segment: everything after the SOS header up to, not including, EOI
    int32_t nbytes;
    int32_t n_mcu;
    int32_t luma_blocks;        // hs * vs blocks of component 0 per MCU ...
    int32_t chroma;             // ... followed by one block each of components 1 and 2 (0 for one component)
    int32_t restart_interval;   // MCUs between RSTn markers, 0: none
    const JpegHuff* dc[3];
    const JpegHuff* ac[3];
};

// coef: n_mcu * (luma_blocks + 2 * chroma) blocks of 64 int16 in natural (row-major) order, in decode order, ZEROED by
// the caller: only non-zero positions are stored.  Values are the quantised coefficients (DC prediction undone),
// truncated to 16 bits.  Returns a JPEG_STATUS_*; after a failure the blocks not reached stay zero.
JPEG_HD int jpeg_decode_scan(const JpegScan& s, int16_t* coef) {
    JpegBits b;
    b.p = s.data;
    b.pos = 0;
    b.end = s.nbytes;
    b.acc = 0;
    b.n = b.pad = b.marker = b.overrun = 0;
    b.cache = 0;
    b.cache_pos = -8;
    // the six table pointers as values: selected by comparisons below, never through an indexed (memory) access
    const JpegHuff *dc0 = s.dc[0], *dc1 = s.dc[1], *dc2 = s.dc[2], *ac0 = s.ac[0], *ac1 = s.ac[1], *ac2 = s.ac[2];
    const int bpm = s.luma_blocks + (s.chroma ? 2 : 0);
    const long n_blocks = (long)s.n_mcu * bpm;
    uint32_t pred0 = 0, pred1 = 0, pred2 = 0;     // unsigned: wraps instead of overflowing on a hostile stream
    long blk = 0;
    int r = 0, mcu = 0, k = 0, restarts = 0;
    for (long it = 0; it < 64 * n_blocks && blk < n_blocks; ++it) {
        const int comp = r < s.luma_blocks ? 0 : 1 + (r - s.luma_blocks);
        jpeg_refill(b);
        if (k == 0) {
            const JpegHuff* h = comp == 0 ? dc0 : (comp == 1 ? dc1 : dc2);
            const int t = jpeg_symbol(b, h);
            if (t < 0) return JPEG_STATUS_BAD_CODE;
            if (b.overrun) return JPEG_STATUS_NO_DATA;
            if (t > 15) return JPEG_STATUS_BAD_DC;
            const uint32_t diff = t ? (uint32_t)jpeg_receive_extend(b, t) : 0u;
            uint32_t p;
            if (comp == 0) p = pred0 += diff;
            else if (comp == 1) p = pred1 += diff;
            else p = pred2 += diff;
            if (b.overrun) return JPEG_STATUS_NO_DATA;
            coef[blk * 64] = (int16_t)(uint16_t)p;
            k = 1;
        } else {
            const JpegHuff* h = comp == 0 ? ac0 : (comp == 1 ? ac1 : ac2);
            const int rs = jpeg_symbol(b, h);
            if (rs < 0) return JPEG_STATUS_BAD_CODE;
            if (b.overrun) return JPEG_STATUS_NO_DATA;
            const int run = rs >> 4, size = rs & 15;
            if (size == 0) {
                if (run == 15) {
                    k += 16;
                    if (k > 64) return JPEG_STATUS_BAD_RUN;
                } else {
                    k = 64;                                   // end of block
                }
            } else {
                k += run;
                if (k > 63) return JPEG_STATUS_BAD_RUN;
                const int v = jpeg_receive_extend(b, size);
                if (b.overrun) return JPEG_STATUS_NO_DATA;
                coef[blk * 64 + jpeg_zigzag(k)] = (int16_t)v;
                ++k;
            }
        }
        if (k >= 64) {
            k = 0;
            ++blk;
            if (++r == bpm) {
                r = 0;
                ++mcu;
                if (s.restart_interval > 0 && mcu < s.n_mcu && mcu % s.restart_interval == 0) {
                    if (!jpeg_take_restart(b, restarts)) return JPEG_STATUS_BAD_RESTART;
                    ++restarts;
                    pred0 = pred1 = pred2 = 0;
                }
            }
        }
    }
    return blk == n_blocks ? JPEG_STATUS_OK : JPEG_STATUS_NO_DATA;
}
