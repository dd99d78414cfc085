// Runs the progressive entropy decoder of instaorder_amd/csrc/jpeg_prog.h -- the code the device kernel compiles -- on the
// CPU under the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I instaorder_amd/csrc \
//       tests/jpeg_prog_host.cpp -o jpeg_prog_host && ./jpeg_prog_host image.bin [...]
//
// (tests/test_jpeg_prog_cpu.py writes the image files from tests/golden/jpeg_prog_cases.npz, builds and runs this.)  Every
// image is decoded as it is; then, for each of its scans, with that scan truncated at every byte (every kStride-th byte for
// an image of more than kEveryByte scan bytes) and with kMutations seeded single-byte mutations of that scan, the other scans
// intact.  All scans of an image run, each stops at its own fault, and the image's status is the first non-zero scan status
// in file order: what the device reports.  The data of a scan and the coefficients live in heap blocks of exactly their
// size, so a read or write one byte outside them is an error.  A line per run:
// "<image> <kind> <scan> <index> <status> <checksum>", kind I (intact), T (first <index> bytes), M (mutation <index>).
//
// An image file is little-endian: int32 magic 0x4a505047, W, H, n_comp, hs, vs, n_tables, n_scans; n_tables x (16 counts, 256
// symbols); per scan 11 int32 (nbytes, n_scan_comp, comp, ss, se, ah, al, restart_interval, tab[3] (-1: none)); then the
// entropy-coded bytes of the scans, one after the other.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_prog.h"

namespace {

constexpr int kEveryByte = 4096, kStride = 16, kMutations = 64;

// the mutation of tests/jpeg_entropy_host.cpp: byte (r % nbytes) becomes (r >> 8) & 255 with r = (m + 1) * 2654435761 mod 2^32
void mutate(uint8_t* d, int nbytes, unsigned m) {
    const uint32_t r = (uint32_t)((m + 1u) * 2654435761u);
    d[r % (uint32_t)nbytes] = (uint8_t)((r >> 8) & 255u);
}

struct Scan {
    int32_t nbytes, n_scan_comp, comp, ss, se, ah, al, restart_interval, tab[3];
    std::vector<uint8_t> data;
};

struct ImageFile {
    int32_t W, H, n_comp, hs, vs;
    std::vector<JpegHuff> huff;
    std::vector<Scan> scans;
    long total_bytes;
};

bool load(const char* path, ImageFile* im) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int32_t head[8];
    bool ok = fread(head, 4, 8, f) == 8 && head[0] == 0x4a505047;
    if (ok) {
        im->W = head[1]; im->H = head[2]; im->n_comp = head[3]; im->hs = head[4]; im->vs = head[5];
        ok = im->W >= 1 && im->W <= 4096 && im->H >= 1 && im->H <= 4096 && (im->n_comp == 1 || im->n_comp == 3) &&
             im->hs >= 1 && im->hs <= 2 && im->vs >= 1 && im->vs <= 2 && head[6] >= 0 && head[6] <= 4096 && head[7] >= 1 &&
             head[7] <= 4096;
    }
    if (ok) {
        im->huff.resize((size_t)head[6]);
        for (int t = 0; t < head[6] && ok; ++t) {
            uint8_t tab[272];
            ok = fread(tab, 272, 1, f) == 1 && jpeg_build_huff(tab, tab + 16, &im->huff[(size_t)t]);
        }
    }
    if (ok) {
        im->scans.resize((size_t)head[7]);
        im->total_bytes = 0;
        for (Scan& s : im->scans) {
            int32_t w[11];
            ok = ok && fread(w, 4, 11, f) == 11;
            if (!ok) break;
            s.nbytes = w[0]; s.n_scan_comp = w[1]; s.comp = w[2]; s.ss = w[3]; s.se = w[4]; s.ah = w[5]; s.al = w[6];
            s.restart_interval = w[7];
            for (int j = 0; j < 3; ++j) s.tab[j] = w[8 + j];
            ok = s.nbytes >= 0 && s.nbytes < (1 << 24) && (s.n_scan_comp == 1 || s.n_scan_comp == im->n_comp) && s.comp >= 0 &&
                 s.comp < im->n_comp && s.ss >= 0 && s.ss <= s.se && s.se <= 63 && s.al >= 0 && s.al <= 13 && s.ah >= 0 &&
                 s.ah <= 14 && s.restart_interval >= 0;
            for (int j = 0; j < 3; ++j) ok = ok && s.tab[j] >= -1 && s.tab[j] < head[6];
            im->total_bytes += s.nbytes;
        }
        for (Scan& s : im->scans) {
            if (!ok) break;
            s.data.resize((size_t)s.nbytes);
            ok = s.nbytes == 0 || fread(s.data.data(), 1, (size_t)s.nbytes, f) == (size_t)s.nbytes;
        }
    }
    fclose(f);
    return ok;
}

// all scans of the image in file order, scan `which` from (bytes, nbytes) in place of its own
int run(const ImageFile& im, int which, const uint8_t* bytes, int nbytes, uint32_t* checksum) {
    const int mw = (im.W + 8 * im.hs - 1) / (8 * im.hs), mh = (im.H + 8 * im.vs - 1) / (8 * im.vs);
    const long n_coef = 64L * mw * mh * (im.hs * im.vs + (im.n_comp == 3 ? 2 : 0));
    int16_t* coef = (int16_t*)calloc((size_t)n_coef, sizeof(int16_t));     // exact size: the sanitizer sees any access outside
    int first = 0;
    static const JpegHuff none = JpegHuff();
    for (size_t n = 0; n < im.scans.size(); ++n) {
        const Scan& s = im.scans[n];
        const uint8_t* src = (int)n == which ? bytes : s.data.data();
        const int len = (int)n == which ? nbytes : s.nbytes;
        uint8_t* data = (uint8_t*)malloc(len > 0 ? (size_t)len : 1);
        if (len > 0) memcpy(data, src, (size_t)len);
        JpegProgScan sc;
        sc.data = data;
        sc.nbytes = len;
        sc.n_scan_comp = s.n_scan_comp;
        sc.comp = s.comp;
        sc.ss = s.ss; sc.se = s.se; sc.ah = s.ah; sc.al = s.al;
        sc.restart_interval = s.restart_interval;
        for (int j = 0; j < 3; ++j) sc.tab[j] = s.tab[j] >= 0 ? &im.huff[(size_t)s.tab[j]] : &none;
        sc.W = im.W; sc.H = im.H; sc.n_comp = im.n_comp; sc.hs = im.hs; sc.vs = im.vs;
        const int st = jpeg_prog_decode_scan(sc, coef);
        if (first == 0) first = st;
        free(data);
    }
    uint32_t sum = 0;
    for (long i = 0; i < n_coef; ++i) sum = sum * 31u + (uint16_t)coef[i];
    *checksum = sum;
    free(coef);
    return first;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s image.bin [...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        ImageFile im;
        if (!load(argv[a], &im)) {
            fprintf(stderr, "%s: not an image file\n", argv[a]);
            return 2;
        }
        uint32_t sum = 0;
        const int intact = run(im, -1, nullptr, 0, &sum);
        printf("%d I 0 0 %d %u\n", a - 1, intact, sum);
        if (intact != JPEG_STATUS_OK) {
            fprintf(stderr, "%s: the intact image does not decode (status %d)\n", argv[a], intact);
            return 1;
        }
        const int step = im.total_bytes > kEveryByte ? kStride : 1;
        for (size_t n = 0; n < im.scans.size(); ++n) {
            const Scan& s = im.scans[n];
            for (int len = 0; len < s.nbytes; len += step) {
                const int st = run(im, (int)n, s.data.data(), len, &sum);
                printf("%d T %zu %d %d %u\n", a - 1, n, len, st, sum);
            }
            if (s.nbytes == 0) continue;
            for (unsigned m = 0; m < (unsigned)kMutations; ++m) {
                std::vector<uint8_t> d = s.data;
                mutate(d.data(), s.nbytes, m);
                const int st = run(im, (int)n, d.data(), s.nbytes, &sum);
                printf("%d M %zu %u %d %u\n", a - 1, n, m, st, sum);
            }
        }
    }
    return 0;
}
