// Runs the parallel entropy scheme of instaorder_amd/csrc/jpeg_sync.h -- the code the device kernels compile -- on the CPU
// under the sanitizers, with the lanes simulated in order (jpeg_sync_decode_scan):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I instaorder_amd/csrc \
//       tests/jpeg_parallel_host.cpp -o jpeg_parallel_host && ./jpeg_parallel_host stream.bin [...]
//
// (tests/test_jpeg_parallel_cpu.py writes the stream files, builds and runs this.)  The stream files and the mutation are
// those of tests/jpeg_entropy_host.cpp.  Every stream is decoded at 16 and at 256 bytes per subsequence: as it is (with as
// many rounds as it has subsequences, and with 2), truncated at every 7th byte and with the first 200 seeded single-byte
// mutations.  The data, the coefficients and the subsequence records live in heap blocks of exactly their size.  A line
// per run: "<stream> <subseq_bytes> <kind> <index> <max_rounds> <rounds> <fallback bits> <status> <checksum>", kind I
// (intact), T (first <index> bytes), M (mutation <index>).  Every run is also decoded by jpeg_decode_scan alone; a
// difference in status or coefficients ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_sync.h"

namespace {

void mutate(uint8_t* d, int nbytes, unsigned m) {
    const uint32_t r = (uint32_t)((m + 1u) * 2654435761u);
    d[r % (uint32_t)nbytes] = (uint8_t)((r >> 8) & 255u);
}

struct Stream {
    int32_t nbytes, n_mcu, luma_blocks, chroma, restart_interval, dc[3], ac[3];
    JpegHuff huff[4];
    std::vector<uint8_t> data;
};

bool load(const char* path, Stream* s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int32_t head[12];
    uint8_t tab[4][272];
    bool ok = fread(head, 4, 12, f) == 12 && head[0] == 0x4a504547 && fread(tab, 272, 4, f) == 4;
    if (ok) {
        s->nbytes = head[1]; s->n_mcu = head[2]; s->luma_blocks = head[3]; s->chroma = head[4]; s->restart_interval = head[5];
        for (int c = 0; c < 3; ++c) { s->dc[c] = head[6 + c] & 3; s->ac[c] = head[9 + c] & 3; }
        ok = s->nbytes > 0 && s->nbytes < (1 << 24) && s->n_mcu > 0 && s->n_mcu < (1 << 20) && s->luma_blocks >= 1 &&
             s->luma_blocks <= 4;
    }
    if (ok) {
        s->data.resize((size_t)s->nbytes);
        ok = fread(s->data.data(), 1, (size_t)s->nbytes, f) == (size_t)s->nbytes;
        for (int t = 0; t < 4 && ok; ++t) ok = jpeg_build_huff(tab[t], tab[t] + 16, &s->huff[t]);
    }
    fclose(f);
    return ok;
}

// false: the parallel scheme and jpeg_decode_scan disagree
bool run(int stream, const Stream& s, const uint8_t* bytes, int nbytes, int subseq, int max_rounds, char kind, int index) {
    uint8_t* data = (uint8_t*)malloc(nbytes > 0 ? (size_t)nbytes : 1);
    if (nbytes > 0) memcpy(data, bytes, (size_t)nbytes);
    const long n_coef = 64L * s.n_mcu * (s.luma_blocks + (s.chroma ? 2 : 0));
    int16_t* coef = (int16_t*)calloc((size_t)n_coef, sizeof(int16_t));
    int16_t* ref = (int16_t*)calloc((size_t)n_coef, sizeof(int16_t));
    const int32_t nsub = jpeg_sync_count(nbytes, subseq);
    uint32_t* rec = (uint32_t*)malloc((size_t)JS_WORDS * nsub * sizeof(uint32_t));
    memset(rec, 0xA5, (size_t)JS_WORDS * nsub * sizeof(uint32_t));
    JpegScan sc;
    sc.data = data;
    sc.nbytes = nbytes;
    sc.n_mcu = s.n_mcu;
    sc.luma_blocks = s.luma_blocks;
    sc.chroma = s.chroma;
    sc.restart_interval = s.restart_interval;
    for (int c = 0; c < 3; ++c) { sc.dc[c] = &s.huff[s.dc[c]]; sc.ac[c] = &s.huff[s.ac[c]]; }
    if (max_rounds <= 0) max_rounds = nsub;
    int status = -1;
    const int32_t info = jpeg_sync_decode_scan(sc, subseq, max_rounds, rec, coef, &status);
    const int want = jpeg_decode_scan(sc, ref);
    const bool same = status == want && memcmp(coef, ref, (size_t)n_coef * sizeof(int16_t)) == 0 && (status == 0 || (info >> 16) != 0);
    uint32_t sum = 0;
    for (long i = 0; i < n_coef; ++i) sum = sum * 31u + (uint16_t)coef[i];
    printf("%d %d %c %d %d %d %d %d %u\n", stream, subseq, kind, index, max_rounds, info & 0xffff, info >> 16, status, sum);
    free(rec);
    free(ref);
    free(coef);
    free(data);
    return same;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s stream.bin [...]\n", argv[0]);
        return 2;
    }
    bool ok = true;
    for (int a = 1; a < argc; ++a) {
        Stream s;
        if (!load(argv[a], &s)) {
            fprintf(stderr, "%s: not a stream file\n", argv[a]);
            return 2;
        }
        for (int subseq : {16, 256}) {
            ok = run(a - 1, s, s.data.data(), s.nbytes, subseq, 0, 'I', 0) && ok;
            ok = run(a - 1, s, s.data.data(), s.nbytes, subseq, 2, 'I', 0) && ok;
            for (int len = 0; len < s.nbytes; len += 7) ok = run(a - 1, s, s.data.data(), len, subseq, 0, 'T', len) && ok;
            for (unsigned m = 0; m < 200; ++m) {
                std::vector<uint8_t> d = s.data;
                mutate(d.data(), s.nbytes, m);
                ok = run(a - 1, s, d.data(), s.nbytes, subseq, 0, 'M', (int)m) && ok;
            }
        }
    }
    if (!ok) fprintf(stderr, "the parallel scheme and jpeg_decode_scan disagree on a run\n");
    return ok ? 0 : 1;
}
