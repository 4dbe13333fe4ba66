// Stand-alone sanitizer program for the blob bookkeeping on the CPU: every case of tests/blob_book_cases.py (dumped to a file by
// profiles/asan_blob_book.sh) through oracle/c/prune.c and through the host instantiation of csrc/blobprune.h (roam_prune_blobs),
// built with -fsanitize=address,undefined.  Exit code 0: no report, and the two agree on every case.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int64_t oracle_prune_blobs(double *blobs, int64_t n, double overlap);
extern "C" int32_t roam_prune_blobs(const double *blobs, int32_t n, double overlap, uint8_t *keep_out);

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) { fprintf(stderr, "usage: asan_blob_book <cases file>\n"); return 2; }
    int32_t ncase = 0, bad = 0;
    if (fread(&ncase, 4, 1, f) != 1) return 2;
    for (int c = 0; c < ncase; c++) {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) return 2;
        std::vector<double> b(3 * (size_t)n + 3), o;
        if (n && fread(b.data(), sizeof(double) * 3, (size_t)n, f) != (size_t)n) return 2;
        o = b;
        std::vector<uint8_t> keep((size_t)n + 1, 0);
        const int64_t kept = oracle_prune_blobs(o.data(), n, 0.5);
        const int32_t rc = roam_prune_blobs(b.data(), n, 0.5, keep.data());
        int64_t diff = 0, kept_host = 0;
        for (int i = 0; i < n; i++) { kept_host += keep[i]; diff += (o[3 * i + 2] > 0) != (keep[i] != 0); }
        printf("case %2d: %5d blobs, oracle keeps %5lld, host keeps %5lld (rc %d), %lld differ\n", c, n, (long long)kept, (long long)kept_host, rc,
               (long long)diff);
        bad += kept < 0 || rc != 0 || diff != 0;
    }
    fclose(f);
    printf("%d of %d cases differ or failed\n", bad, ncase);
    return bad ? 1 : 0;
}
