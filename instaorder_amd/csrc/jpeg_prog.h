// Progressive JPEG entropy decoder of ONE scan (ITU T.81 G.1.2), written once for the device kernel (csrc/jpeg.hip) and for a
// host program that runs it under the sanitizers (tests/jpeg_prog_host.cpp).  Built on the bit reader and the Huffman tables
// of jpeg_entropy.h; no HIP header is needed: with a plain C++ compiler the functions are ordinary inline functions.
//
// A progressive file sends its coefficients over many scans; each scan names a band Ss..Se of the zig-zag order and a bit
// position Al, and is one of four kinds, all handled here:
//   DC first       (Ss = 0, Ah = 0)  a DC difference per block as in a baseline scan, stored shifted left by Al
//   DC refinement  (Ss = 0, Ah > 0)  one plain bit per block: bit Al of the DC value
//   AC first       (Ss > 0, Ah = 0)  run/size symbols inside the band, values shifted left by Al; a symbol EOBn ends the
//                                    band of this block and of the next EOBRUN - 1 blocks
//   AC refinement  (Ss > 0, Ah > 0)  symbols of size 1 place a new coefficient of magnitude 1 << Al behind `run` still-zero
//                                    positions; every coefficient that is already non-zero and is passed on the way takes one
//                                    correction bit; ZRL passes 16 zero positions; EOBn as above, the blocks of the run still
//                                    take their correction bits
// A scan of all components walks the MCUs of the image; a scan of one component walks that component's own raster of
// ceil(w_c / 8) x ceil(h_c / 8) blocks (narrower than the padded MCU grid when the size is no multiple of the MCU), an MCU
// being one block.  Restart intervals count the scan's own MCUs; predictions and EOBRUN are reset at every restart.
//
// The work is bounded whatever the bytes are: the block loop runs once per block of the scan; inside a block every pass of a
// symbol loop moves k forward by at least one or leaves the loop, so a block decodes at most Se - Ss + 2 symbols and visits
// every coefficient position of its band at most once; EOBRUN is at most (1 << 14) + (1 << 14) - 1 = 32767.  Bytes are read
// at positions [0, nbytes) only (the reader of jpeg_entropy.h), past the end it supplies zero bits and using one flags the
// scan.  A coefficient is stored at block * 64 + zigzag[k] with block < n_blocks and Ss <= k <= Se <= 63 checked first.  The
// (at most three) table pointers are selected by comparisons, never through an indexed (memory) access.
#pragma once
#include "jpeg_entropy.h"

struct JpegProgScan {
    const uint8_t* data;        // the entropy-coded segment of the scan: the bytes after its SOS header up to the next marker
    int32_t nbytes;
    int32_t n_scan_comp;        // components of the scan: 1, or all components of the image
    int32_t comp;               // the component of a one-component scan (frame order)
    int32_t ss, se, ah, al;     // 0 <= ss <= se <= 63, al <= 13 (the caller checked)
    int32_t restart_interval;   // MCUs of THIS scan between RSTn markers, 0: none
    const JpegHuff* tab[3];     // per scan component: the DC table (DC first) or the AC table (AC scans); unused otherwise
    int32_t W, H, n_comp, hs, vs;   // the image: 1 component, or 3 with luma sampling hs x vs and chroma 1 x 1
};

// one correction bit for the non-zero coefficient *c
JPEG_HD void jpeg_prog_correct(JpegBits& b, int16_t* c, int al) {
    jpeg_refill(b);
    const int bit = (int)jpeg_peek(b, 1);
    jpeg_skip(b, 1);
    const int v = *c;
    if (bit && (v & (1 << al)) == 0) *c = (int16_t)(v >= 0 ? v + (1 << al) : v - (1 << al));
}

// coef: the image's n_mcu * blocks_per_mcu blocks of 64 int16 in natural (row-major) order, in MCU order, zeroed by the
// caller before the image's FIRST scan; the scans of an image run in an order that respects their levels.  Returns a
// JPEG_STATUS_*; after a failure the blocks not reached keep what earlier scans left.
JPEG_HD int jpeg_prog_decode_scan(const JpegProgScan& s, int16_t* coef) {
    JpegBits b;
    b.p = s.data;
    b.pos = 0;
    b.end = s.nbytes;
    b.acc = 0;
    b.n = b.pad = b.marker = b.overrun = 0;
    b.cache = 0;
    b.cache_pos = -8;
    const JpegHuff *t0 = s.tab[0], *t1 = s.tab[1], *t2 = s.tab[2];
    const int ss = s.ss & 63, se = s.se & 63, al = s.al & 15;
    const int luma = s.hs * s.vs;
    const int bpm = luma + (s.n_comp == 3 ? 2 : 0);
    const int mw = (s.W + 8 * s.hs - 1) / (8 * s.hs), mh = (s.H + 8 * s.vs - 1) / (8 * s.vs);
    const long n_blocks = (long)mw * mh * bpm;
    const bool interleaved = s.n_scan_comp > 1;
    // the raster of a one-component scan
    const int ch = s.comp == 0 ? s.hs : 1, cv = s.comp == 0 ? s.vs : 1;
    const int bw = ((s.W * ch + s.hs - 1) / s.hs + 7) / 8, bh = ((s.H * cv + s.vs - 1) / s.vs + 7) / 8;
    const long scan_blocks = interleaved ? n_blocks : (long)bw * bh;
    const int per_mcu = interleaved ? bpm : 1;
    const long n_mcu = scan_blocks / per_mcu;
    const int p1 = 1 << al;
    uint32_t pred0 = 0, pred1 = 0, pred2 = 0;     // unsigned: wraps instead of overflowing on a hostile stream
    int eobrun = 0, restarts = 0, r = 0, bx = 0, by = 0;
    long mcu = 0;
    for (long n = 0; n < scan_blocks; ++n) {
        long blk;
        int j;                                     // which of the scan's components
        if (interleaved) {
            blk = n;
            j = r < luma ? 0 : 1 + (r - luma);
        } else {
            const int rr = s.comp == 0 ? (by % cv) * ch + bx % ch : luma + s.comp - 1;
            blk = ((long)(by / cv) * mw + bx / ch) * bpm + rr;
            j = 0;
        }
        if (blk < 0 || blk >= n_blocks) return JPEG_STATUS_NO_DATA;      // cannot happen for the geometry above
        int16_t* c = coef + blk * 64;
        jpeg_refill(b);
        if (ss == 0 && s.ah == 0) {                                      // DC first
            const JpegHuff* h = j == 0 ? t0 : (j == 1 ? t1 : t2);
            const int t = jpeg_symbol(b, h);
            if (t < 0) return JPEG_STATUS_BAD_CODE;
            if (b.overrun) return JPEG_STATUS_NO_DATA;
            if (t > 15) return JPEG_STATUS_BAD_DC;
            const uint32_t diff = t ? (uint32_t)jpeg_receive_extend(b, t) : 0u;
            uint32_t p;
            if (j == 0) p = pred0 += diff;
            else if (j == 1) p = pred1 += diff;
            else p = pred2 += diff;
            if (b.overrun) return JPEG_STATUS_NO_DATA;
            c[0] = (int16_t)(uint16_t)(p << al);
        } else if (ss == 0) {                                            // DC refinement
            const int bit = (int)jpeg_peek(b, 1);
            jpeg_skip(b, 1);
            if (b.overrun) return JPEG_STATUS_NO_DATA;
            if (bit) c[0] = (int16_t)(c[0] | p1);
        } else if (s.ah == 0) {                                          // AC first
            if (eobrun > 0) {
                --eobrun;
            } else {
                int k = ss;
                while (k <= se) {
                    jpeg_refill(b);
                    const int rs = jpeg_symbol(b, t0);
                    if (rs < 0) return JPEG_STATUS_BAD_CODE;
                    if (b.overrun) return JPEG_STATUS_NO_DATA;
                    const int run = rs >> 4, size = rs & 15;
                    if (size) {
                        k += run;
                        if (k > se) return JPEG_STATUS_BAD_RUN;
                        const int v = jpeg_receive_extend(b, size);
                        if (b.overrun) return JPEG_STATUS_NO_DATA;
                        c[jpeg_zigzag(k)] = (int16_t)(uint16_t)((uint32_t)v << al);
                        ++k;
                    } else if (run == 15) {
                        k += 16;
                        if (k > se + 1) return JPEG_STATUS_BAD_RUN;
                    } else {
                        eobrun = 1 << run;
                        if (run) {
                            eobrun += (int)jpeg_peek(b, run);
                            jpeg_skip(b, run);
                            if (b.overrun) return JPEG_STATUS_NO_DATA;
                        }
                        --eobrun;                                        // this block is the first of the run
                        break;
                    }
                }
            }
        } else {                                                         // AC refinement
            int k = ss;
            if (eobrun == 0) {
                while (k <= se) {
                    jpeg_refill(b);
                    const int rs = jpeg_symbol(b, t0);
                    if (rs < 0) return JPEG_STATUS_BAD_CODE;
                    if (b.overrun) return JPEG_STATUS_NO_DATA;
                    int run = rs >> 4;
                    const int size = rs & 15;
                    int value = 0;
                    if (size) {
                        if (size != 1) return JPEG_STATUS_BAD_CODE;
                        value = jpeg_peek(b, 1) ? p1 : -p1;
                        jpeg_skip(b, 1);
                        if (b.overrun) return JPEG_STATUS_NO_DATA;
                    } else if (run != 15) {
                        eobrun = 1 << run;
                        if (run) {
                            eobrun += (int)jpeg_peek(b, run);
                            jpeg_skip(b, run);
                            if (b.overrun) return JPEG_STATUS_NO_DATA;
                        }
                        break;
                    }
                    // over the coefficients that are known (one correction bit each) and `run` that are still zero
                    while (k <= se) {
                        int16_t* q = c + jpeg_zigzag(k);
                        if (*q != 0) {
                            jpeg_prog_correct(b, q, al);
                        } else if (--run < 0) {
                            break;
                        }
                        ++k;
                    }
                    if (b.overrun) return JPEG_STATUS_NO_DATA;
                    if (value) {
                        if (k > se) return JPEG_STATUS_BAD_RUN;
                        c[jpeg_zigzag(k)] = (int16_t)value;
                    }
                    ++k;
                }
            }
            if (eobrun > 0) {
                for (; k <= se; ++k) {
                    int16_t* q = c + jpeg_zigzag(k);
                    if (*q != 0) jpeg_prog_correct(b, q, al);
                }
                if (b.overrun) return JPEG_STATUS_NO_DATA;
                --eobrun;
            }
        }
        // the next block of the scan, and a restart marker where an interval of the scan's MCUs ends
        bool mcu_done = true;
        if (interleaved) {
            if (++r == bpm) r = 0;
            else mcu_done = false;
        } else if (++bx == bw) {
            bx = 0;
            ++by;
        }
        if (mcu_done) {
            ++mcu;
            if (s.restart_interval > 0 && mcu < n_mcu && mcu % s.restart_interval == 0) {
                if (!jpeg_take_restart(b, restarts)) return JPEG_STATUS_BAD_RESTART;
                ++restarts;
                pred0 = pred1 = pred2 = 0;
                eobrun = 0;
            }
        }
    }
    return JPEG_STATUS_OK;
}
