// csrc/png_inflate_par.h on the CPU, for the sanitizers (tests/test_png_parallel_cpu.py builds this with
// -fsanitize=address,undefined).  usage: png_parallel_host FILE CHUNK_BYTES...: records of <int32 magic, int32 nbytes,
// int32 expected> + nbytes DEFLATE bytes (tests/png_cases.py host_records).  Every stream goes through the steps of
// io_png_decode_par at every chunk size with the waves simulated in order, one lane each -- search and count for every
// chunk, the chain, then either store, tail and head for the chain chunks or the sequential png_inflate, as the predicate
// says -- and is compared with png_inflate alone, byte for byte and status for status.  The data and every workspace region
// (records, symbols, scanlines, the second ring) live in heap blocks of exactly their sizes, so a read or a write outside
// them stops the run.  One line per stream and size: index, chunk_bytes, info word, status, 1 if stored in parallel.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_inflate_par.h"

template <typename T>
static T* exact(size_t count) {                               // a heap block of exactly count elements (one byte for none)
    return static_cast<T*>(malloc(count ? count * sizeof(T) : 1));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + got);
    fclose(f);
    PngShared* sh = static_cast<PngShared*>(aligned_alloc(16, sizeof(PngShared)));
    size_t at = 0;
    int index = 0, failures = 0;
    while (at + 12 <= all.size()) {
        int32_t head[3];
        memcpy(head, all.data() + at, 12);
        at += 12;
        if (head[0] != 0x474e5089 || head[1] < 0 || head[2] < 0 || at + (size_t)head[1] > all.size()) return 3;
        const long nbytes = head[1], expected = head[2];
        uint8_t* block = exact<uint8_t>(nbytes);
        memcpy(block, all.data() + at, nbytes);
        at += nbytes;
        const uint8_t* data = nbytes ? block : block + 1;
        const size_t room = ((size_t)expected + 15) / 16 * 16;   // the workspace range of the kernels is padded to 16 bytes
        uint8_t* want = static_cast<uint8_t*>(aligned_alloc(16, room ? room : 16));
        memset(sh, 0xA5, sizeof(PngShared));
        const int want_status = png_inflate(sh, data, nbytes, want, expected, 0, 1);
        for (int a = 2; a < argc; ++a) {
            const int chunk_bytes = atoi(argv[a]);
            if (chunk_bytes < PNG_PAR_MIN_CHUNK || chunk_bytes > PNG_PAR_MAX_CHUNK || chunk_bytes % PNG_PAR_MIN_CHUNK) return 2;
            const int nchunks = (int)png_par_chunks(nbytes, chunk_bytes);
            PngParRec* recs = exact<PngParRec>(nchunks);
            uint16_t* syms = exact<uint16_t>(expected);
            uint8_t* lines = static_cast<uint8_t*>(aligned_alloc(16, room ? room : 16));
            uint8_t* hi = exact<uint8_t>(PNG_RING_BYTES);
            memset(lines, 0x5A, room);
            for (int c = 0; c < nchunks; ++c) {                 // png_par_search_kernel
                memset(sh, 0xA5, sizeof(PngShared));
                long cand = 0;
                if (c > 0) {
                    const long lo = 8L * c * chunk_bytes, end = 8L * nbytes;
                    cand = png_par_search(sh, data, nbytes, lo, lo + 8L * chunk_bytes < end ? lo + 8L * chunk_bytes : end, 0, 1);
                }
                recs[c] = PngParRec{cand, 0, 0, -1, 0, PNG_EXIT_NONE, 0, -1};
            }
            for (int c = 0; c < nchunks; ++c) {                 // png_par_count_kernel
                if (recs[c].cand < 0) continue;
                memset(sh, 0xA5, sizeof(PngShared));
                PngParOut r;
                png_par_decode<false>(sh, nullptr, data, nbytes, (long)recs[c].cand, expected, recs, nchunks, chunk_bytes, nullptr, 0,
                                      r, 0, 1);
                recs[c].exit_bit = r.exit_bit; recs[c].n = r.n; recs[c].reach = r.reach; recs[c].exit = r.exit;
                recs[c].status = r.status; recs[c].next = r.next;
            }
            const int info = png_par_chain(recs, nchunks, expected);
            int par = (info >> 16) == 0, status = 0;
            if (par) {
                for (int c = 0; c < nchunks; ++c) {             // png_par_store_kernel
                    const PngParRec rec = recs[c];
                    if (rec.offset < 0 || rec.offset + rec.n > expected) continue;
                    memset(sh, 0xA5, sizeof(PngShared));
                    memset(hi, 0xA5, PNG_RING_BYTES);
                    PngParOut r;
                    png_par_decode<true>(sh, hi, data, nbytes, (long)rec.cand, expected, recs, nchunks, chunk_bytes, syms + rec.offset,
                                         (long)rec.n, r, 0, 1);
                    if (r.exit != rec.exit || r.exit_bit != rec.exit_bit || r.n != rec.n || r.reach != rec.reach) par = 0;
                }
            }
            if (par) {
                png_par_tail(recs, nchunks, expected, syms, lines, 0, 1);
                for (int c = 0; c < nchunks; ++c)               // png_par_head_kernel, three shares per chunk
                    if (recs[c].offset >= 0 && recs[c].offset + recs[c].n <= expected)
                        for (int part = 0; part < 3; ++part) png_par_head(recs[c], syms, lines, part, 3);
            } else {
                memset(sh, 0xA5, sizeof(PngShared));
                status = png_inflate(sh, data, nbytes, lines, expected, 0, 1);
            }
            if (status != want_status || (status == 0 && memcmp(lines, want, expected) != 0)) {
                fprintf(stderr, "stream %d at %d bytes: status %d (sequential %d) or other bytes\n", index, chunk_bytes, status,
                        want_status);
                ++failures;
            }
            printf("%d %d %d %d %d\n", index, chunk_bytes, info, status, par);
            free(recs);
            free(syms);
            free(lines);
            free(hi);
        }
        ++index;
        free(block);
        free(want);
    }
    free(sh);
    if (failures) return 4;
    return at == all.size() ? 0 : 3;
}
