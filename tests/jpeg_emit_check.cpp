// Stand-alone check of the JPEG encoder's host stage, linked with csrc/jpeg_emit.cpp alone and built by
// tests/test_jpeg_encode_host.py with -fsanitize=address,undefined: ssd_jpeg_emit writes into a caller's buffer of a caller's size,
// so this is where its memory safety is checked.
//
//   jpeg_emit_check CORPUS
// CORPUS (tests/helpers/jpeg_enc_cases.write_corpus): per case int32 {height, width, sampling, quality, sweep}, int64 n, int16 [n]
// coefficients, int64 size, the expected file.  Every case runs with exact-size heap copies: the coefficients in a buffer of n
// values, the output in a buffer of `size` bytes -- a read or a write one byte outside is the sanitizer's to report -- and must
// give the expected bytes.  A case marked `sweep` also runs every capacity from 0 to ssd_jpeg_emit_bound - 1, each in a heap
// buffer of exactly that size: SSD_OK with the expected bytes from `size` on, SSD_ERR_INVALID below.
// Prints "cases N sweeps M capacities K"; the exit status is 0 unless a result was wrong.
#include "../include/ssd_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// one call with an output buffer of exactly `cap` bytes: the status, and whether the bytes are the expected ones
static int run(const int16_t *coef, const int32_t *head, int64_t cap, const std::vector<uint8_t> &want, bool *equal)
{
    uint8_t *out = (uint8_t *)malloc(cap ? (size_t)cap : 1);
    int64_t size = -1;
    const int rc = ssd_jpeg_emit(coef, head[0], head[1], head[2], head[3], cap ? out : nullptr, cap, &size);
    *equal = rc == SSD_OK && size == (int64_t)want.size() && memcmp(out, want.data(), want.size()) == 0;
    free(out);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "%s: cannot open\n", argv[1]);
        return 2;
    }
    long cases = 0, sweeps = 0, capacities = 0, bad = 0;
    int32_t head[5];
    while (fread(head, sizeof(int32_t), 5, f) == 5) {
        int64_t n = 0, size = 0;
        if (!read_exact(f, &n, sizeof(n)) || n < 0) return 2;
        int16_t *coef = (int16_t *)malloc((size_t)n * sizeof(int16_t) + (n ? 0 : 1));      // exact size: the value behind is not ours
        if (!read_exact(f, coef, (size_t)n * sizeof(int16_t)) || !read_exact(f, &size, sizeof(size)) || size < 0) return 2;
        std::vector<uint8_t> want((size_t)size);
        if (!read_exact(f, want.data(), want.size())) return 2;
        const int64_t bound = ssd_jpeg_emit_bound(head[0], head[1], head[2]);
        bool equal = false;
        if (bound < size || run(coef, head, size, want, &equal) != SSD_OK || !equal) {
            fprintf(stderr, "case %ld (%d x %d, %d, q %d): the exact-size run failed (bound %lld, size %lld)\n", cases, head[0], head[1],
                    head[2], head[3], (long long)bound, (long long)size);
            ++bad;
        }
        if (head[4]) {
            for (int64_t cap = 0; cap < bound; ++cap, ++capacities) {
                const int rc = run(coef, head, cap, want, &equal);
                if (cap >= size ? (rc != SSD_OK || !equal) : rc != SSD_ERR_INVALID) {
                    fprintf(stderr, "case %ld: capacity %lld of size %lld gave status %d\n", cases, (long long)cap, (long long)size, rc);
                    ++bad;
                }
            }
            ++sweeps;
        }
        free(coef);
        ++cases;
    }
    fclose(f);
    printf("cases %ld sweeps %ld capacities %ld\n", cases, sweeps, capacities);
    return bad ? 1 : 0;
}
