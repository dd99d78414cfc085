// Entropy decoding of ONE baseline JPEG scan on many lanes, by self-synchronisation of the Huffman stream (DESIGN.md "JPEG
// images", parallel entropy stage).  Written once for the device kernels (csrc/jpeg.hip) and for a host program that runs it
// under the sanitizers (tests/jpeg_parallel_host.cpp); ``JpegImage.parallel_plan`` (instaorder_amd/jpeg.py) is the same rule
// in Python.  The tables (JpegHuff) and the scan description (JpegScan) are those of jpeg_entropy.h.
//
// The raw entropy bytes are cut into subsequences of `subseq_bytes` bytes.  The SCAN STATE at a point is (byte, bit, r, k, m):
// the raw index of the byte unit (a byte, or FF 00) that holds the next unread bit and how many of its bits are used, the
// block index in the MCU, the coefficient index, and the MCUs since the last restart (0 without a restart interval).
//
//   rounds   Round 1: subsequence 0 starts from the true initial state, every other one from a guess at its first byte
//            (jpeg_sync_guess).  A subsequence is decoded WITHOUT storing anything (jpeg_sync_decode<false>) until the next
//            unread bit lies at or past its end, or the data ends; the exit state and what the pass counted are recorded.
//            Round t decodes again exactly the subsequences whose entry state -- the predecessor's exit after round t - 1 --
//            changed.  Rounds end when no entry changed or after max_rounds.  All entries of a round are taken before any
//            subsequence is decoded, so the result does not depend on the order in which lanes run.
//   lenient  A speculative decode never aborts: bits that are no code skip one bit, a run past coefficient 63 ends the
//            block, a DC category above 15 counts as 0.  RSTn is a hard synchronisation point: whatever the state, decoding
//            goes on behind it, byte-aligned, with r = k = m = 0 and the predictions reset.  Each such event is a VIOLATION,
//            recorded (with the number of blocks completed before it) beside the state, never in it.  Data that ends is no
//            violation, it ends the decode.  Every pass uses at least one bit, so a decode makes at most 8 * subseq_bytes + 32
//            passes whatever the bytes are.
//   finish   (jpeg_sync_finish, one lane) An exclusive prefix sum of the block counts gives each subsequence its first
//            block; the live range ends with the subsequence in which the count reaches n_blocks.  The image is CLEAN when
//            the rounds converged, no violation happened before block n_blocks, the restart markers met before block
//            n_blocks count 0, 1, 2 ... modulo 8, and the data held n_blocks blocks.  The chain of converged decodes of a clean image is
//            the sequential decode of jpeg_decode_scan, symbol by symbol.
//   write    (jpeg_sync_decode<true>) Every live subsequence of a clean image is decoded once more from its entry state,
//            with its first block and its DC predictions (prefix sums of the DC differences, segmented at restarts), and
//            stores what jpeg_decode_scan stores.  Every other image is left to jpeg_decode_scan.
//
// Safety does not depend on the bytes: reads are at [0, nbytes) only, table indices are masked, a coefficient is stored at
// block * 64 + zigzag[k] with block < n_blocks and k <= 63 checked first, and every loop has a bound given by the caller.
#pragma once
#include "jpeg_entropy.h"

#define JPEG_SYNC_MIN_BYTES 16
#define JPEG_SYNC_MAX_BYTES 4096
#define JPEG_SYNC_MAX_ROUNDS 65535
#define JPEG_INFO_NOT_CONVERGED (1 << 16)
#define JPEG_INFO_NOT_CLEAN (1 << 17)

// The record of subsequence i is the words rec[w * nsub + i]: a lane's stores are never adjacent, so none is wider than 4 bytes
enum {
    JS_E_BYTE, JS_E_BRK, JS_E_M, JS_CHANGED,                     // entry state (brk = bit | r << 8 | k << 16), decode it again
    JS_X_BYTE, JS_X_BRK, JS_X_M,                                 // exit state
    JS_BLOCKS,                                                   // blocks completed
    JS_DC01, JS_DC2D,                                            // DC difference sums since the last restart (16 bits each); bits 16-18 of DC2D: marker delta
    JS_NRST, JS_RSTBLK,                                          // restart markers passed; blocks completed before the first
    JS_VIOL,                                                     // blocks completed before the first violation, -1: none
    JS_FIRST, JS_PRED01, JS_PRED2,                               // finish: first block, DC predictions at the entry
    JS_WORDS
};

JPEG_HD bool jpeg_sync_params_ok(int subseq_bytes, int max_rounds) {
    return subseq_bytes >= JPEG_SYNC_MIN_BYTES && subseq_bytes <= JPEG_SYNC_MAX_BYTES && subseq_bytes % 8 == 0 &&
           max_rounds >= 1 && max_rounds <= JPEG_SYNC_MAX_ROUNDS;
}

JPEG_HD int32_t jpeg_sync_count(int32_t nbytes, int subseq_bytes) {
    return nbytes <= 0 ? 1 : (int32_t)(((int64_t)nbytes + subseq_bytes - 1) / subseq_bytes);
}

// ---- bit reader that knows where it is ----------------------------------------------------------------------------------
struct JpegSyncBits {
    const uint8_t* p;
    int32_t end, pos;   // pos: the next raw byte to take
    uint64_t acc;       // the low n bits are the unread bits, all real
    int32_t n;
    uint32_t hist;      // bit j: the j-th youngest byte of acc was an FF 00 pair
    int32_t stall;      // 0; 1: the data ends at pos (or with a lone FF); 2: p[pos] = FF in front of something other than 00
};

// n >= 32 afterwards unless the reader stalls; at most four bytes are added
JPEG_HD void jpeg_sync_refill(JpegSyncBits& b) {
    if (b.n >= 32 || b.stall) return;
    if (b.pos + 4 <= b.end) {
        uint32_t w;
        memcpy(&w, b.p + b.pos, 4);
        const uint32_t x = ~w;
        if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {       // no byte of w is FF
            b.acc = (b.acc << 32) | __builtin_bswap32(w);
            b.n += 32;
            b.hist <<= 4;
            b.pos += 4;
            return;
        }
    }
    for (int i = 0; i < 4 && b.n < 32; ++i) {
        if (b.pos >= b.end) { b.stall = 1; return; }
        const uint32_t byte = b.p[b.pos];
        if (byte != 0xFF) {
            b.acc = (b.acc << 8) | byte;
            b.hist <<= 1;
            b.pos += 1;
        } else {
            if (b.pos + 1 >= b.end) { b.stall = 1; return; }
            if (b.p[b.pos + 1] != 0) { b.stall = 2; return; }
            b.acc = (b.acc << 8) | 0xFFu;
            b.hist = (b.hist << 1) | 1u;
            b.pos += 2;
        }
        b.n += 8;
    }
}

// raw index of the byte unit that holds the next unread bit (pos when nothing is buffered)
JPEG_HD int32_t jpeg_sync_byte(const JpegSyncBits& b) {
    const int nb = (b.n + 7) >> 3;                               // <= 8
    return b.pos - nb - __builtin_popcount(b.hist & ((1u << nb) - 1u));
}

// the next 32 bits, zeros behind the buffered ones
JPEG_HD uint32_t jpeg_sync_window(const JpegSyncBits& b) {
    return b.n >= 32 ? (uint32_t)(b.acc >> (b.n - 32)) : (uint32_t)(b.acc << (32 - b.n));
}

// symbol and length of the code that starts the 16 bits c16, or -1
JPEG_HD int jpeg_sync_code(const JpegHuff* h, uint32_t c16, int* len) {
    const uint32_t e = h->look[(c16 >> (16 - JPEG_LOOKUP_BITS)) & 255u];
    if (e) {
        *len = (int)(e >> 8);
        return (int)(e & 255u);
    }
    for (int l = JPEG_LOOKUP_BITS + 1; l <= 16; ++l) {
        const int c = (int)(c16 >> (16 - l));
        if (c <= h->maxcode[l]) {
            *len = l;
            return h->sym[(h->valoff[l] + c) & 255];
        }
    }
    return -1;
}

struct JpegSyncOut {
    int32_t byte;
    uint32_t brk;
    int32_t m, blocks;
    uint32_t dc0, dc1, dc2;
    int32_t nrst, rst_delta, rst_blocks, viol;
};

// the guess for subsequence i >= 1: its first byte, stepped over the 00 of an FF 00 pair and the code of an RSTn that straddle the boundary
JPEG_HD int32_t jpeg_sync_guess(const uint8_t* p, int32_t nbytes, int32_t i, int subseq_bytes) {
    const int64_t g64 = (int64_t)i * subseq_bytes;
    int32_t g = g64 < nbytes ? (int32_t)g64 : nbytes;
    if (g >= 1 && g < nbytes && p[g - 1] == 0xFF && (p[g] == 0 || (p[g] & 0xF8) == 0xD0)) ++g;
    return g;
}

// One subsequence from the entry state (e_byte, e_brk, e_m) up to raw byte sub_end.  STORE = false: count only.  STORE = true:
// the write pass, blocks from first_block on, predictions p0..p2, stops at n_blocks.
template <bool STORE>
JPEG_HD void jpeg_sync_decode(const JpegScan& s, int32_t sub_end, int32_t max_passes, int32_t e_byte, uint32_t e_brk,
                              int32_t e_m, int16_t* coef, long first_block, long n_blocks, uint32_t p0, uint32_t p1,
                              uint32_t p2, JpegSyncOut* out) {
    const JpegHuff *dc0 = s.dc[0], *dc1 = s.dc[1], *dc2 = s.dc[2], *ac0 = s.ac[0], *ac1 = s.ac[1], *ac2 = s.ac[2];
    const int luma = s.luma_blocks, bpm = s.luma_blocks + (s.chroma ? 2 : 0), ri = s.restart_interval;
    JpegSyncBits b;
    b.p = s.data;
    b.end = s.nbytes;
    b.pos = e_byte < 0 ? 0 : (e_byte > s.nbytes ? s.nbytes : e_byte);
    b.acc = 0;
    b.n = 0;
    b.hist = 0;
    b.stall = 0;
    int r = (int)((e_brk >> 8) & 255u), k = (int)((e_brk >> 16) & 255u), m = e_m;
    if (r >= bpm) r = 0;
    if (k > 63) k = 0;
    int32_t blocks = 0, nrst = 0, rst_delta = 0, rst_blocks = 0, viol = -1;
    uint32_t d0 = 0, d1 = 0, d2 = 0;
    jpeg_sync_refill(b);
    {
        const int bit = (int)(e_brk & 7u);
        if (bit && b.n >= 8) b.n -= bit;
    }
    int32_t pass = 0;
    for (; pass < max_passes; ++pass) {
        if (STORE && first_block + blocks >= n_blocks) break;
        jpeg_sync_refill(b);
        if (b.pos >= sub_end && jpeg_sync_byte(b) >= sub_end) break;
        int what = 0;                                            // 1: the reader stands at FF xx and the bits in front of it are dropped
        if (ri > 0 && r == 0 && k == 0 && m >= ri) {             // a restart interval is complete
            if (b.n >= 8) {                                      // data where the marker should be
                if (viol < 0) viol = blocks;
                m = 0;
            } else if (b.stall == 1) {
                break;
            } else {
                what = 1;
            }
        }
        if (!what) {
            const uint32_t w = jpeg_sync_window(b);
            const int comp = r < luma ? 0 : 1 + (r - luma);
            const JpegHuff* h = k == 0 ? (comp == 0 ? dc0 : (comp == 1 ? dc1 : dc2)) : (comp == 0 ? ac0 : (comp == 1 ? ac1 : ac2));
            int len = 0;
            const int sym = jpeg_sync_code(h, w >> 16, &len);
            if (sym < 0 && !(b.stall && b.n < 16)) {             // no code: skip a bit
                if (viol < 0) viol = blocks;
                b.n -= 1;
                continue;
            }
            int size = k == 0 ? sym : (sym & 15);
            if (k == 0 && sym > 15) {
                if (viol < 0) viol = blocks;
                size = 0;
            }
            if (sym < 0 || len + size > b.n) {                   // the symbol needs bits the reader does not have: it stalls
                if (b.stall != 2) break;                         // the data ends
                if (viol < 0) viol = blocks;                     // a marker inside an interval
                what = 1;
            } else {
                const int v = size ? (int)((w << len) >> (32 - size)) : 0;
                const int val = size ? (v >= (1 << (size - 1)) ? v : v - (1 << size) + 1) : 0;
                b.n -= len + size;
                const long blk = first_block + blocks;
                if (k == 0) {
                    uint32_t pr;
                    if (comp == 0) { d0 += (uint32_t)val; pr = p0 += (uint32_t)val; }
                    else if (comp == 1) { d1 += (uint32_t)val; pr = p1 += (uint32_t)val; }
                    else { d2 += (uint32_t)val; pr = p2 += (uint32_t)val; }
                    if (STORE && blk < n_blocks) coef[blk * 64] = (int16_t)(uint16_t)pr;
                    k = 1;
                } else {
                    const int run = sym >> 4;
                    if (size == 0) {
                        if (run == 15) {
                            k += 16;
                            if (k > 64) {
                                if (viol < 0) viol = blocks;
                                k = 64;
                            }
                        } else {
                            k = 64;
                        }
                    } else {
                        k += run;
                        if (k > 63) {
                            if (viol < 0) viol = blocks;
                            k = 64;
                        } else {
                            if (STORE && blk < n_blocks) coef[blk * 64 + jpeg_zigzag(k)] = (int16_t)val;
                            ++k;
                        }
                    }
                }
                if (k >= 64) {
                    k = 0;
                    ++blocks;
                    if (++r >= bpm) {
                        r = 0;
                        if (ri > 0) ++m;
                    }
                }
                continue;
            }
        }
        // the reader stands at FF xx, xx != 00, inside the data (stall == 2): the bits in front of it are dropped
        if (b.stall != 2) break;                                 // (p[pos + 1] exists only there)
        const uint32_t x = b.p[b.pos + 1];
        if (x == 0xFF) {                                       // a fill byte
            b.pos += 1;
        } else if ((x & 0xF8u) == 0xD0u) {                       // RSTn: the hard synchronisation point
            const int32_t d = (int32_t)((x - (uint32_t)nrst) & 7u);
            if (nrst == 0) {
                rst_delta = d;
                rst_blocks = blocks;
            } else if (d != rst_delta && viol < 0) {
                viol = blocks;
            }
            ++nrst;
            b.pos += 2;
            r = k = m = 0;
            d0 = d1 = d2 = 0;
            p0 = p1 = p2 = 0;
        } else {                                                 // any other marker ends the data
            if (viol < 0) viol = blocks;
            break;
        }
        b.n = 0;
        b.hist = 0;
        b.stall = 0;
    }
    if (pass >= max_passes && viol < 0) viol = blocks;           // cannot happen: every pass uses a bit of the subsequence
    out->byte = jpeg_sync_byte(b);
    out->brk = (uint32_t)((8 - (b.n & 7)) & 7) | ((uint32_t)r << 8) | ((uint32_t)k << 16);
    out->m = m;
    out->blocks = blocks;
    out->dc0 = d0;
    out->dc1 = d1;
    out->dc2 = d2;
    out->nrst = nrst;
    out->rst_delta = rst_delta;
    out->rst_blocks = rst_blocks;
    out->viol = viol;
}

// ---- the steps of the scheme on the records of one image ----------------------------------------------------------------
JPEG_HD int32_t jpeg_sync_end_of(const JpegScan& s, int32_t i, int subseq_bytes) {
    const int64_t e = ((int64_t)i + 1) * subseq_bytes;
    return e < s.nbytes ? (int32_t)e : s.nbytes;
}

JPEG_HD void jpeg_sync_init_one(const JpegScan& s, uint32_t* rec, int32_t nsub, int32_t i, int subseq_bytes) {
    rec[(size_t)JS_E_BYTE * nsub + i] = i == 0 ? 0u : (uint32_t)jpeg_sync_guess(s.data, s.nbytes, i, subseq_bytes);
    rec[(size_t)JS_E_BRK * nsub + i] = 0u;
    rec[(size_t)JS_E_M * nsub + i] = 0u;
    rec[(size_t)JS_CHANGED * nsub + i] = 1u;
}

// decode subsequence i if its entry changed
JPEG_HD void jpeg_sync_round_one(const JpegScan& s, uint32_t* rec, int32_t nsub, int32_t i, int subseq_bytes) {
    if (!rec[(size_t)JS_CHANGED * nsub + i]) return;
    JpegSyncOut o;
    jpeg_sync_decode<false>(s, jpeg_sync_end_of(s, i, subseq_bytes), 8 * subseq_bytes + 32, (int32_t)rec[(size_t)JS_E_BYTE * nsub + i],
                            rec[(size_t)JS_E_BRK * nsub + i], (int32_t)rec[(size_t)JS_E_M * nsub + i], nullptr, 0, 0, 0u, 0u, 0u, &o);
    rec[(size_t)JS_X_BYTE * nsub + i] = (uint32_t)o.byte;
    rec[(size_t)JS_X_BRK * nsub + i] = o.brk;
    rec[(size_t)JS_X_M * nsub + i] = (uint32_t)o.m;
    rec[(size_t)JS_BLOCKS * nsub + i] = (uint32_t)o.blocks;
    rec[(size_t)JS_DC01 * nsub + i] = (o.dc0 & 0xffffu) | (o.dc1 << 16);
    rec[(size_t)JS_DC2D * nsub + i] = (o.dc2 & 0xffffu) | ((uint32_t)o.rst_delta << 16);
    rec[(size_t)JS_NRST * nsub + i] = (uint32_t)o.nrst;
    rec[(size_t)JS_RSTBLK * nsub + i] = (uint32_t)o.rst_blocks;
    rec[(size_t)JS_VIOL * nsub + i] = (uint32_t)o.viol;
}

// the entry of subsequence i >= 1 becomes its predecessor's exit; true if that changed it.  i = 0 never changes.
JPEG_HD bool jpeg_sync_entry_one(uint32_t* rec, int32_t nsub, int32_t i) {
    if (i == 0) {
        rec[(size_t)JS_CHANGED * nsub] = 0u;
        return false;
    }
    const uint32_t nb = rec[(size_t)JS_X_BYTE * nsub + i - 1], nk = rec[(size_t)JS_X_BRK * nsub + i - 1],
                   nm = rec[(size_t)JS_X_M * nsub + i - 1];
    const bool ch = nb != rec[(size_t)JS_E_BYTE * nsub + i] || nk != rec[(size_t)JS_E_BRK * nsub + i] ||
                    nm != rec[(size_t)JS_E_M * nsub + i];
    rec[(size_t)JS_E_BYTE * nsub + i] = nb;
    rec[(size_t)JS_E_BRK * nsub + i] = nk;
    rec[(size_t)JS_E_M * nsub + i] = nm;
    rec[(size_t)JS_CHANGED * nsub + i] = ch ? 1u : 0u;
    return ch;
}

// after convergence, one lane: first blocks and predictions of the live range; returns the number of live subsequences, or 0
// for an image that is not clean
JPEG_HD int32_t jpeg_sync_finish(uint32_t* rec, int32_t nsub, long n_blocks) {
    long first = 0;
    uint32_t p0 = 0, p1 = 0, p2 = 0, markers = 0;
    bool clean = true, full = false;
    int32_t live = 0;
    for (int32_t i = 0; i < nsub && !full; ++i) {
        rec[(size_t)JS_FIRST * nsub + i] = (uint32_t)first;
        rec[(size_t)JS_PRED01 * nsub + i] = (p0 & 0xffffu) | (p1 << 16);
        rec[(size_t)JS_PRED2 * nsub + i] = p2 & 0xffffu;
        const int32_t viol = (int32_t)rec[(size_t)JS_VIOL * nsub + i], nrst = (int32_t)rec[(size_t)JS_NRST * nsub + i];
        const uint32_t dc01 = rec[(size_t)JS_DC01 * nsub + i], dc2d = rec[(size_t)JS_DC2D * nsub + i];
        if (viol >= 0 && first + viol < n_blocks) clean = false;
        if (nrst > 0) {
            if (first + (int32_t)rec[(size_t)JS_RSTBLK * nsub + i] < n_blocks && ((dc2d >> 16) & 7u) != (markers & 7u)) clean = false;
            markers += (uint32_t)nrst;
            p0 = p1 = p2 = 0;
        }
        p0 += dc01 & 0xffffu;
        p1 += dc01 >> 16;
        p2 += dc2d & 0xffffu;
        first += (int32_t)rec[(size_t)JS_BLOCKS * nsub + i];
        live = i + 1;
        full = first >= n_blocks;
    }
    return clean && full ? live : 0;
}

// the write pass of live subsequence i of a clean image
JPEG_HD void jpeg_sync_write_one(const JpegScan& s, const uint32_t* rec, int32_t nsub, int32_t i, int subseq_bytes, int16_t* coef,
                                 long n_blocks) {
    JpegSyncOut o;
    const uint32_t p01 = rec[(size_t)JS_PRED01 * nsub + i];
    jpeg_sync_decode<true>(s, jpeg_sync_end_of(s, i, subseq_bytes), 8 * subseq_bytes + 32, (int32_t)rec[(size_t)JS_E_BYTE * nsub + i],
                           rec[(size_t)JS_E_BRK * nsub + i], (int32_t)rec[(size_t)JS_E_M * nsub + i], coef,
                           (long)rec[(size_t)JS_FIRST * nsub + i], n_blocks, p01 & 0xffffu, p01 >> 16,
                           rec[(size_t)JS_PRED2 * nsub + i], &o);
}

// The whole scheme with the lanes simulated in order (the host program; the kernels run the same steps side by side).
// rec: JS_WORDS * nsub words.  coef as for jpeg_decode_scan, zeroed.  Returns the info word: bits 0-15 the rounds run, bit 16
// not converged, bit 17 not clean; *status is what jpeg_decode_scan returns for an image that falls back, else 0.
JPEG_HD int32_t jpeg_sync_decode_scan(const JpegScan& s, int subseq_bytes, int max_rounds, uint32_t* rec, int16_t* coef, int* status) {
    const int32_t nsub = jpeg_sync_count(s.nbytes, subseq_bytes);
    const long n_blocks = (long)s.n_mcu * (s.luma_blocks + (s.chroma ? 2 : 0));
    for (int32_t i = 0; i < nsub; ++i) jpeg_sync_init_one(s, rec, nsub, i, subseq_bytes);
    int32_t rounds = 0;
    bool converged = false;
    for (int t = 1; t <= max_rounds && !converged; ++t) {
        for (int32_t i = 0; i < nsub; ++i) jpeg_sync_round_one(s, rec, nsub, i, subseq_bytes);
        rounds = t;
        bool any = false;
        for (int32_t i = 0; i < nsub; ++i) any = jpeg_sync_entry_one(rec, nsub, i) || any;
        converged = !any;
    }
    int32_t info = rounds;
    int32_t live = 0;
    if (!converged) info |= JPEG_INFO_NOT_CONVERGED;
    else if ((live = jpeg_sync_finish(rec, nsub, n_blocks)) == 0) info |= JPEG_INFO_NOT_CLEAN;
    if (info >> 16) {
        *status = jpeg_decode_scan(s, coef);
    } else {
        for (int32_t i = 0; i < live; ++i) jpeg_sync_write_one(s, rec, nsub, i, subseq_bytes, coef, n_blocks);
        *status = JPEG_STATUS_OK;
    }
    return info;
}
