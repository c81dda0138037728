// Stand-alone check of the JPEG decoder's host stage, linked with csrc/jpeg_host.cpp alone and built by tests/test_jpeg_host.py
// with -fsanitize=address,undefined: the parser eats untrusted bytes, so this is where its memory safety is checked.
//
//   jpeg_host_check FILE... [--refused FILE...]
// For every file: the file itself, every proper prefix, and every single-byte change (three values) at each of the first 700
// bytes go through ssd_jpeg_info_read and, when that accepts, ssd_jpeg_entropy.  Every input is an exact-size heap copy and the
// two output buffers are sized exactly as `info` says, so a read or a write one byte outside is the sanitizer's to report.
// Prints "FILE: runs N accepted M" per file; the exit status is 0 unless a prefix was accepted or the untouched file was not.
// A file behind --refused is one the parser takes and ssd_jpeg_entropy refuses as not pinned (the exact passes of a loud block run
// on it): untouched it must give SSD_ERR_UNSUPPORTED, and its line ends "accepted M refused".
#include "../include/ssd_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int run(const uint8_t *data, size_t n)
{
    uint8_t *copy = (uint8_t *)malloc(n ? n : 1);       // exact size: the byte behind the input is not ours
    memcpy(copy, data, n);
    ssd_jpeg_info info;
    int rc = ssd_jpeg_info_read(copy, (int64_t)n, &info);
    if (rc == SSD_OK) {
        int16_t *coef = (int16_t *)malloc((size_t)info.coef_count * sizeof(int16_t));
        uint16_t *quant = (uint16_t *)malloc((size_t)info.components * 64 * sizeof(uint16_t));
        rc = ssd_jpeg_entropy(copy, (int64_t)n, &info, coef, quant);
        free(coef);
        free(quant);
    }
    free(copy);
    return rc;
}

int main(int argc, char **argv)
{
    int bad = 0;
    bool refused = false;       // behind --refused: the untouched file is one ssd_jpeg_entropy refuses
    for (int a = 1; a < argc; ++a) {
        if (strcmp(argv[a], "--refused") == 0) {
            refused = true;
            continue;
        }
        FILE *f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + got);
        fclose(f);
        long runs = 0, accepted = 0;
        const int whole = run(d.data(), d.size());
        if (whole != (refused ? SSD_ERR_UNSUPPORTED : SSD_OK)) {
            fprintf(stderr, "%s: the untouched file gave status %d\n", argv[a], whole);
            ++bad;
        }
        ++runs, accepted += whole == SSD_OK;
        for (size_t n = 0; n < d.size(); ++n, ++runs) {
            const int rc = run(d.data(), n);
            if (rc != SSD_ERR_INVALID && rc != SSD_ERR_UNSUPPORTED) {
                fprintf(stderr, "%s: the first %zu bytes gave status %d\n", argv[a], n, rc);
                ++bad;
            }
        }
        std::vector<uint8_t> m = d;
        for (size_t p = 0; p < d.size() && p < 700; ++p) {
            const uint8_t vals[3] = {(uint8_t)(d[p] ^ 0xFF), (uint8_t)(d[p] + 1), 0xFF};
            for (uint8_t v : vals) {
                m[p] = v;
                const int rc = run(m.data(), m.size());
                if (rc == SSD_OK) ++accepted;
                else if (rc != SSD_ERR_INVALID && rc != SSD_ERR_UNSUPPORTED) {
                    fprintf(stderr, "%s: byte %zu = %u gave status %d\n", argv[a], p, (unsigned)v, rc);
                    ++bad;
                }
                ++runs;
            }
            m[p] = d[p];
        }
        printf("%s: runs %ld accepted %ld%s\n", argv[a], runs, accepted, refused ? " refused" : "");
    }
    return bad ? 1 : 0;
}
