// csrc/png_inflate.h on the CPU, for the sanitizers (tests/test_png_cpu.py builds this with -fsanitize=address,undefined).
// usage: png_inflate_host FILE: records of <int32 magic, int32 nbytes, int32 expected> + nbytes DEFLATE bytes
// (tests/png_cases.py host_records).  Every stream is inflated by the header's loop with one lane; the data and the output
// live in heap blocks of exactly their sizes, so a read or a write outside them stops the run.  One line per stream:
// index, status, Adler-32 of the output (by the header's split sums, over three uneven shares) or 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_inflate.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + got);
    fclose(f);
    PngShared* sh = static_cast<PngShared*>(aligned_alloc(16, sizeof(PngShared)));
    size_t at = 0;
    int index = 0;
    while (at + 12 <= all.size()) {
        int32_t head[3];
        memcpy(head, all.data() + at, 12);
        at += 12;
        if (head[0] != 0x474e5089 || head[1] < 0 || head[2] < 0 || at + (size_t)head[1] > all.size()) return 3;
        uint8_t* data = static_cast<uint8_t*>(malloc(head[1] ? head[1] : 1));
        memcpy(data, all.data() + at, head[1]);
        at += head[1];
        const size_t room = ((size_t)head[2] + 15) / 16 * 16;      // the workspace range of the kernel is padded to 16 bytes
        uint8_t* dst = static_cast<uint8_t*>(aligned_alloc(16, room ? room : 16));
        memset(sh, 0xA5, sizeof(PngShared));
        const int status = png_inflate(sh, head[1] ? data : data + 1, head[1], dst, head[2], 0, 1);
        uint32_t adler = 0;
        if (status == 0) {
            uint64_t s1 = 0, s2 = 0;
            const long n = head[2], cuts[4] = {0, n / 5, n / 5 + (n - n / 5) / 3, n};
            for (int k = 0; k < 3; ++k) {
                uint64_t a = 0, b = 0;
                for (long i = cuts[k]; i < cuts[k + 1]; ++i) { a += dst[i]; b += (uint64_t)i * dst[i]; }
                s1 += a % 65521;
                s2 += b % 65521;
            }
            adler = png_adler_finish(s1, s2, (uint64_t)n);
        }
        printf("%d %d %u\n", index++, status, adler);
        free(data);
        free(dst);
    }
    free(sh);
    return at == all.size() ? 0 : 3;
}
