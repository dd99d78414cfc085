// Runs the entropy decoder of instaorder_amd/csrc/jpeg_entropy.h -- the code the device kernel compiles -- on the CPU under
// the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I instaorder_amd/csrc \
//       tests/jpeg_entropy_host.cpp -o jpeg_entropy_host && ./jpeg_entropy_host stream.bin [...]
//
// (tests/test_jpeg_cpu.py writes the stream files from tests/golden/jpeg_cases.npz, builds and runs this.)  Every stream is
// decoded as it is, truncated at every byte, and with 1000 seeded single-byte mutations.  The data and the coefficients live
// in heap blocks of exactly their size, so a read or write one byte outside them is an error.  A line per run:
// "<stream> <kind> <index> <status> <checksum>", kind I (intact), T (first <index> bytes), M (mutation <index>).
//
// A stream file is little-endian: int32 magic 0x4a504547, nbytes, n_mcu, luma_blocks, chroma, restart_interval, dc[3],
// ac[3] (indices into the four tables), then 4 x (16 counts, 256 symbols), then the entropy-coded bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"

namespace {

// the mutation the GPU test repeats in Python: byte (r % nbytes) becomes (r >> 8) & 255 with r = (m + 1) * 2654435761 mod 2^32
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

int run(const Stream& s, const uint8_t* bytes, int nbytes, uint32_t* checksum) {
    // exact-size heap blocks: the sanitizer sees any access outside them
    uint8_t* data = (uint8_t*)malloc(nbytes > 0 ? (size_t)nbytes : 1);
    if (nbytes > 0) memcpy(data, bytes, (size_t)nbytes);
    const long n_coef = 64L * s.n_mcu * (s.luma_blocks + (s.chroma ? 2 : 0));
    int16_t* coef = (int16_t*)calloc((size_t)n_coef, sizeof(int16_t));
    JpegScan sc;
    sc.data = data;
    sc.nbytes = nbytes;
    sc.n_mcu = s.n_mcu;
    sc.luma_blocks = s.luma_blocks;
    sc.chroma = s.chroma;
    sc.restart_interval = s.restart_interval;
    for (int c = 0; c < 3; ++c) { sc.dc[c] = &s.huff[s.dc[c]]; sc.ac[c] = &s.huff[s.ac[c]]; }
    const int status = jpeg_decode_scan(sc, coef);
    uint32_t sum = 0;
    for (long i = 0; i < n_coef; ++i) sum = sum * 31u + (uint16_t)coef[i];
    *checksum = sum;
    free(coef);
    free(data);
    return status;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s stream.bin [...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        Stream s;
        if (!load(argv[a], &s)) {
            fprintf(stderr, "%s: not a stream file\n", argv[a]);
            return 2;
        }
        uint32_t sum = 0;
        const int intact = run(s, s.data.data(), s.nbytes, &sum);
        printf("%d I 0 %d %u\n", a - 1, intact, sum);
        if (intact != JPEG_STATUS_OK) {
            fprintf(stderr, "%s: the intact stream does not decode (status %d)\n", argv[a], intact);
            return 1;
        }
        for (int len = 0; len < s.nbytes; ++len) {
            const int st = run(s, s.data.data(), len, &sum);
            printf("%d T %d %d %u\n", a - 1, len, st, sum);
        }
        for (unsigned m = 0; m < 1000; ++m) {
            std::vector<uint8_t> d = s.data;
            mutate(d.data(), s.nbytes, m);
            const int st = run(s, d.data(), s.nbytes, &sum);
            printf("%d M %u %d %u\n", a - 1, m, st, sum);
        }
    }
    return 0;
}
