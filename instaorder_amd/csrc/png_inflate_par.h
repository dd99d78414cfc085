// ONE DEFLATE stream inflated on many waves from found block starts (DESIGN.md "Parallel inflate"): the rule of
// io_png_decode_par, written once for the kernels of csrc/png.hip and for a host program that simulates the waves in order
// under the sanitizers (tests/png_parallel_host.cpp).  PngImage.parallel_plan (instaorder_amd/png.py) states it in Python.
//
// Code tables are per block, so a decoder started at a wrong bit never falls into step: parallel work starts at block
// headers only, and correctness never depends on a guess being right.
//   1. search   The DEFLATE bytes are cut into chunks of chunk_bytes.  Chunk 0 starts at bit 0; chunk c >= 1 takes as its
//               candidate the first bit of its own range at which a complete dynamic-block header parses by
//               png_dynamic_header's own rules, all of it inside the data (png_par_search).  No such bit: nothing to do.
//   2. count    Every chunk with a candidate decodes from it block after block and stores nothing (png_par_decode<false>).
//               At a block boundary at bit b: a final block ends the decode ("final"); b being exactly the candidate of a
//               later chunk ends it too ("link"); otherwise the next block follows.  What the sequential loop gives a
//               status word for ends the decode with that word.  A distance past the chunk's own bytes is no error here:
//               reach = the largest (distance - bytes produced so far in this chunk) says how far in front of its first
//               byte the chunk reads.  Output is capped at the image's size (status 7).
//   3. chain    One lane per image walks from chunk 0 along the links and sums the byte counts into output offsets
//               (png_par_chain).  The image is CLEAN when no record on the chain has a status, every reach is at most its
//               chunk's offset, the last exit is "final" and the sum is the expected size.  Chunk 0 starts at the true start
//               and every link is an exact block boundary of the true decode, so the chain of a clean image IS the
//               sequential decode block by block; candidates off the chain are wasted work and nothing else.
//   4. store    The chain chunks of a clean image with at least two of them decode again (png_par_decode<true>) and write
//               16-bit symbols at their offsets: a literal or a byte copied from inside the chunk is its value, a byte from
//               in front of the chunk's first byte is the marker 0x8000 | k for the byte k + 1 positions in front of it
//               (k < 32768).  Matches copy symbols, markers included.  The pass is held to the record (bytes, exit, reach):
//               a symbol past the recorded count is not written, and a pass that disagrees hands the image to the fallback.
//   5. resolve  The bytes a chunk's markers name lie in the last 32768 symbols of the chunks in front of it.  One workgroup
//               per image turns those tails into bytes in chain order (window propagation, png_par_tail); then every other
//               symbol turns into its byte independently (png_par_head).  Bytes land where png_inflate would have put them.
//   6. fallback Every other image -- not clean, a chain of one, no chunk at all -- is inflated by png_inflate, unchanged, in
//               a launch behind these, by a per-image predicate.  Status words and bytes of such streams are therefore the
//               sequential decoder's by construction.
//
// Bounds, none of which depends on the stream bytes.  The search tries 8 * chunk_bytes bits, lanes at a time, and parses at
// most one header per bit.  A decode is the sequential loop with its bounds: at least one bit per symbol and three per block,
// so at most 8 * data_bytes + 64 iterations, reads at [0, data_bytes) only (zeros past the end, status 6), code-length loop
// at most 316 entries.  The chain walk moves to a later chunk at every step: at most `chunks` steps.  A symbol is stored at
// offset + j only for j < the recorded count, and offset + count <= expected was checked by the chain; a marker's byte
// position offset - 1 - k is checked against 0 before the read.
//
// Workspace of io_png_decode_par, in this order (io_png_par_workspace_bytes), with units = sum over the images of
// ceil(H (1 + rowbytes) / 16) and chunks = sum of ceil(data_bytes / chunk_bytes):
//   round16(8 (n + 1))   first 16-byte unit of every image's scanlines    } io_png_workspace_bytes
//   16 units             the scanlines                                    }
//   32 units             the 16-bit symbols
//   round16(8 (n + 1))   first record of every image
//   round16(8 n)         two predicate words per image: stored in parallel, left to the sequential kernel
//   48 chunks            the records (PngParRec)
#pragma once
#include "png_inflate.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_BALLOT(x) ((uint64_t)__ballot(x))
#else
#define PNG_BALLOT(x) ((uint64_t)((x) ? 1 : 0))
#endif

#define PNG_PAR_MIN_CHUNK 256       // chunk_bytes: a multiple of this ...
#define PNG_PAR_MAX_CHUNK (1 << 20) // ... up to this
#define PNG_PAR_MAX_CHUNKS 65535    // chunks of one image
#define PNG_PAR_REC_BYTES 48
#define PNG_INFO_NOT_CLEAN (1 << 16)
#define PNG_INFO_CHAIN_OF_ONE (1 << 17)

enum { PNG_EXIT_NONE = 0, PNG_EXIT_FINAL = 1, PNG_EXIT_LINK = 2, PNG_EXIT_STATUS = 3, PNG_EXIT_MISMATCH = 4 };

struct PngParRec {
    long long cand;      // the chunk's candidate bit, -1: none
    long long exit_bit;  // the bit behind the last block decoded (or where the status arose)
    long long n;         // bytes produced
    long long offset;    // of the chunk's first byte in the image's output; -1: not on the chain
    int32_t reach, exit, status, next;
};
static_assert(sizeof(PngParRec) == PNG_PAR_REC_BYTES, "PngParRec");

PNG_HD size_t png_par_round16(size_t x) { return (x + 15) / 16 * 16; }
PNG_HD long png_par_chunks(long data_bytes, int chunk_bytes) { return (data_bytes + chunk_bytes - 1) / chunk_bytes; }

// 57 bits of the data from `bit` on, first bit lowest, zeros past the end (one lane's own read: the search prefilter)
PNG_HD uint64_t png_par_bits(const uint8_t* data, long nbytes, long bit) {
    const long b = bit >> 3;
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i)
        if (b + i < nbytes) v |= (uint64_t)data[b + i] << (8 * i);
    return v >> (bit & 7);
}

// Necessary for a dynamic-block header at `bit`: BTYPE = 2, HLIT <= 286, HDIST <= 30 and a COMPLETE code-length code
// (Kraft sum exactly 1 over its HCLEN + 4 lengths), which is what png_build(kind 0) accepts.
PNG_HD bool png_par_prefilter(const uint8_t* data, long nbytes, long bit) {
    const uint64_t h = png_par_bits(data, nbytes, bit);
    if (((h >> 1) & 3) != 2) return false;
    if (((h >> 3) & 31) > 29 || ((h >> 8) & 31) > 29) return false;
    const int ncode = (int)((h >> 13) & 15) + 4;
    const uint64_t c = png_par_bits(data, nbytes, bit + 17);
    int kraft = 0;
    for (int i = 0; i < ncode; ++i) {
        const int v = (int)((c >> (3 * i)) & 7);
        if (v) kraft += 128 >> v;
    }
    return kraft == 128;
}

// a reader that starts at `bit` of data[0, nbytes): the bit reader of png_inflate.h over the bytes from bit >> 3 on
PNG_HD void png_par_start(PngInflate& s, PngShared* sh, const uint8_t* data, long nbytes, long bit, int lane, int lanes) {
    const long byte = bit >> 3;
    s.sh = sh; s.data = data + byte; s.nbytes = nbytes - byte; s.dst = nullptr; s.expected = 0; s.lane = lane; s.lanes = lanes;
    s.buf = 0; s.cnt = 0; s.pos = 0; s.out = 0; s.flushed = 0;
    s.win_base = -PNG_WIN_BYTES;
    png_refill(s);
    png_take(s, (int)(bit & 7));
}

// does a complete dynamic-block header parse at `bit`?  Uniform over the wave.
PNG_HD bool png_par_header_at(PngShared* sh, const uint8_t* data, long nbytes, long bit, int lane, int lanes) {
    PngInflate s;
    png_par_start(s, sh, data, nbytes, bit, lane, lanes);
    png_refill(s);
    png_take(s, 1);
    const int type = png_take(s, 2);
    if (png_overrun(s) || type != 2) return false;
    return png_dynamic_header(s) == PNG_STATUS_OK;
}

// the first bit of [lo_bit, hi_bit) at which a dynamic-block header parses, -1: none.  Lanes test different bits; the few
// that pass the prefilter are parsed by the whole wave, in order.  (hi_bit - lo_bit) / lanes rounds, at most `lanes` parses each.
PNG_HD long png_par_search(PngShared* sh, const uint8_t* data, long nbytes, long lo_bit, long hi_bit, int lane, int lanes) {
    for (long base = lo_bit; base < hi_bit; base += lanes) {
        const long p = base + lane;
        uint64_t mask = PNG_BALLOT(p < hi_bit && png_par_prefilter(data, nbytes, p));
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1;
            if (png_par_header_at(sh, data, nbytes, base + j, lane, lanes)) return base + j;
        }
    }
    return -1;
}

struct PngParOut {
    long long exit_bit, n;
    int reach, exit, status, next;
    long blocks[3];      // stored, fixed, dynamic blocks decoded
};

// Decodes from `start_bit` block after block until a final block, a link or a status (the rule above).  cand[0, nchunks):
// the candidates of the image's chunks.  STORE: symbols go to sym[0, limit) (the chunk's range of the image's symbol
// array) and to the rings sh->ring (low bytes) / hi (high bytes, PNG_RING_BYTES of them); a symbol at or past `limit` ends
// the pass with PNG_EXIT_MISMATCH.  Without STORE `sym` and `hi` are not touched.
template <bool STORE>
PNG_HD void png_par_decode(PngShared* sh, uint8_t* hi, const uint8_t* data, long nbytes, long start_bit, long expected,
                           const PngParRec* recs, int nchunks, int chunk_bytes, uint16_t* sym, long limit, PngParOut& r,
                           int lane, int lanes) {
    PngInflate s;
    png_par_start(s, sh, data, nbytes, start_bit, lane, lanes);
    const long byte0 = start_bit >> 3;
    const long chunk_bits = 8L * chunk_bytes;
    const int M = PNG_RING_BYTES - 1;
    long out = 0;
    int reach = 0;
    r.blocks[0] = r.blocks[1] = r.blocks[2] = 0;
    r.next = -1;
    r.status = 0;
#define PNG_PAR_END(kind, st)                                                              \
    {                                                                                      \
        r.exit = (kind); r.status = (st); r.exit_bit = 8 * byte0 + png_bits_used(s);       \
        r.n = out; r.reach = reach;                                                        \
        return;                                                                            \
    }
    for (;;) {                                               // every block consumes at least its 3 header bits
        png_refill(s);
        const int final = png_take(s, 1);
        const int type = png_take(s, 2);
        if (png_overrun(s)) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_NO_DATA)
        if (type == 3) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_BLOCK_TYPE)
        if (type == 0) {
            png_take(s, s.cnt & 7);
            png_refill(s);
            const int len = png_take(s, 16), nlen = png_take(s, 16);
            if (png_overrun(s)) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_NO_DATA)
            if (len != (nlen ^ 0xffff)) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_STORED_LEN)
            s.pos -= s.cnt >> 3;                             // whole bytes that were taken into buf go back
            s.buf = 0;
            s.cnt = 0;
            if (s.pos + len > s.nbytes) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_NO_DATA)
            if (out + len > expected) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_SIZE)
            if (STORE) {
                if (out + len > limit) PNG_PAR_END(PNG_EXIT_MISMATCH, 0)
                for (int done = 0; done < len; done += PNG_FLUSH_BYTES) {    // pieces: no two lanes meet in a ring slot
                    const int piece = len - done < PNG_FLUSH_BYTES ? len - done : PNG_FLUSH_BYTES;
                    for (int i = lane; i < piece; i += lanes) {
                        const uint8_t v = s.data[s.pos + done + i];
                        sh->ring[(out + done + i) & M] = v;
                        hi[(out + done + i) & M] = 0;
                        sym[out + done + i] = v;
                    }
                    PNG_SYNC();
                }
            }
            out += len;
            s.pos += len;
            s.win_base = s.pos - PNG_WIN_BYTES;              // the window is stale: the next refill loads it at pos
            r.blocks[0]++;
        } else {
            if (type == 1) {
                png_build_fixed(s);
            } else {
                const int rc = png_dynamic_header(s);
                if (rc) PNG_PAR_END(PNG_EXIT_STATUS, rc)
            }
            r.blocks[type]++;
            for (;;) {                                       // every symbol consumes at least one bit
                png_refill(s);
                int c = png_symbol(s, sh->lit_look, PNG_LIT_BITS, sh->lit_count, sh->lit_sym);
                if (c < 0) PNG_PAR_END(PNG_EXIT_STATUS, 8 * s.nbytes - png_bits_used(s) < 15 ? PNG_STATUS_NO_DATA : PNG_STATUS_SYMBOL)
                if (png_overrun(s)) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_NO_DATA)
                if (c < 256) {
                    if (out >= expected) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_SIZE)
                    if (STORE) {
                        if (out >= limit) PNG_PAR_END(PNG_EXIT_MISMATCH, 0)
                        if (lane == 0) {
                            sh->ring[out & M] = (uint8_t)c;
                            hi[out & M] = 0;
                            sym[out] = (uint16_t)c;
                        }
                    }
                    out++;
                    continue;
                }
                if (c == 256) break;
                if (c > 285) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_SYMBOL)
                c -= 257;
                const int len = png_len_base(c) + png_take(s, png_len_extra(c));
                png_refill(s);
                const int ds = png_symbol(s, sh->dist_look, PNG_DIST_BITS, sh->dist_count, sh->dist_sym);
                if (ds < 0) PNG_PAR_END(PNG_EXIT_STATUS, 8 * s.nbytes - png_bits_used(s) < 15 ? PNG_STATUS_NO_DATA : PNG_STATUS_SYMBOL)
                if (png_overrun(s)) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_NO_DATA)
                if (ds > 29) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_SYMBOL)
                const int dist = png_dist_base(ds) + png_take(s, png_dist_extra(ds));
                if (png_overrun(s)) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_NO_DATA)
                if (dist > out && (int)(dist - out) > reach) reach = (int)(dist - out);    // dist <= 32768
                if (out + len > expected) PNG_PAR_END(PNG_EXIT_STATUS, PNG_STATUS_SIZE)
                if (STORE) {
                    if (out + len > limit) PNG_PAR_END(PNG_EXIT_MISMATCH, 0)
                    PNG_SYNC();                              // the literals in front of the match are in the rings
                    for (int i = lane; i < len; i += lanes) {
                        const int k = dist >= len ? i : i % dist;       // an overlapping match repeats its first `dist` symbols
                        const long src = out - dist + k;                // < out
                        uint16_t v;
                        if (src < 0) v = (uint16_t)(0x8000 | (-src - 1)); // the byte -src positions in front of the chunk
                        else v = (uint16_t)(sh->ring[src & M] | (hi[src & M] << 8));
                        sym[out + i] = v;                 // sources lie in front of `out`: no lane reads a slot written here
                        sh->ring[(out + i) & M] = (uint8_t)v;
                        hi[(out + i) & M] = (uint8_t)(v >> 8);
                    }
                    PNG_SYNC();
                }
                out += len;
            }
        }
        if (final) PNG_PAR_END(PNG_EXIT_FINAL, 0)
        const long b = 8 * byte0 + png_bits_used(s);
        const long ci = b / chunk_bits;
        if (ci < nchunks && recs[ci].cand == b) {
            r.next = (int)ci;
            PNG_PAR_END(PNG_EXIT_LINK, 0)
        }
    }
#undef PNG_PAR_END
}

// The chain of one image (one lane): output offsets into the records it visits, and the info word -- bits 0..15 the chunks
// visited (the one the walk stopped at included), bit 16 not clean, bit 17 clean but a chain of one.
PNG_HD int png_par_chain(PngParRec* recs, int nchunks, long expected) {
    int count = 0, c = 0;
    bool clean = false;
    long long off = 0;
    while (c < nchunks) {                                    // c grows at every step: at most nchunks of them
        PngParRec& r = recs[c];
        r.offset = off;
        ++count;
        if ((r.exit != PNG_EXIT_FINAL && r.exit != PNG_EXIT_LINK) || r.reach > off || off + r.n > expected) break;
        off += r.n;
        if (r.exit == PNG_EXIT_FINAL) {
            clean = off == expected;
            break;
        }
        if (r.next <= c) break;
        c = r.next;
    }
    int info = count > 65535 ? 65535 : count;
    if (!clean) info |= PNG_INFO_NOT_CLEAN;
    else if (count < 2) info |= PNG_INFO_CHAIN_OF_ONE;
    return info;
}

// symbol j of the chunk at `off` to its byte; a marker's byte was resolved before (it lies in the tail of an earlier chunk)
PNG_HD void png_par_byte(const uint16_t* sym, uint8_t* lines, long long off, long long j) {
    const uint16_t v = sym[off + j];
    uint8_t b = (uint8_t)v;
    if (v & 0x8000) {
        const long long p = off - 1 - (v & 0x7fff);
        b = p >= 0 ? lines[p] : (uint8_t)0;
    }
    lines[off + j] = b;
}

// Window propagation of a clean image: the last PNG_RING_BYTES symbols of every chain chunk, in chain order, by all threads
// of one workgroup (a barrier between chunks: a marker names a byte of an EARLIER chunk's tail).  At most nchunks steps.
PNG_HD void png_par_tail(const PngParRec* recs, int nchunks, long expected, const uint16_t* sym, uint8_t* lines, int tid,
                         int threads) {
    int c = 0;
    for (int step = 0; step < nchunks; ++step) {
        const PngParRec r = recs[c];
        if (r.offset < 0 || r.n < 0 || r.offset + r.n > expected) break;      // never so on a clean chain; uniform over the block
        const long long t0 = r.n > PNG_RING_BYTES ? r.n - PNG_RING_BYTES : 0;
        for (long long j = t0 + tid; j < r.n; j += threads) png_par_byte(sym, lines, r.offset, j);
        PNG_SYNC();
        if (r.exit != PNG_EXIT_LINK || r.next <= c || r.next >= nchunks) break;
        c = r.next;
    }
}

// every symbol of a chain chunk in front of its tail, independently: share `part` of `parts`
PNG_HD void png_par_head(const PngParRec& r, const uint16_t* sym, uint8_t* lines, long part, long parts) {
    const long long t0 = r.n > PNG_RING_BYTES ? r.n - PNG_RING_BYTES : 0;
    for (long long j = part; j < t0; j += parts) png_par_byte(sym, lines, r.offset, j);
}
