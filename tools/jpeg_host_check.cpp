// Stand-alone robustness walk of the JPEG host half (csrc/jpeg_host.cpp), meant to be built with the host compiler and
// -fsanitize=address,undefined (tests/test_jpeg_host.py does): no HIP, no GPU, nothing loaded into another process.
//
//     jpeg_host_check FILE... [--mutate FILE...]
//
// Every FILE must decode; then every proper prefix of it is decoded, and for the files behind --mutate every single-byte change
// (each position, each of the 255 other values).  Each input lives in a heap block of exactly its length, so a read past the
// end is an error the sanitizer sees.  A refusal is fine; the exit status is 0 unless a whole file is refused or a sanitizer
// stops the program.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../lightweight-human-pose-estimation.pytorch_amd/csrc/jpeg_host.h"

static int decode(const unsigned char* d, size_t n, std::vector<int16_t>& coef, char* msg, size_t cap) {
    lwp_jpeg_header hd;
    uint16_t qt[4 * 64];
    int rc = lwp::jpeg_parse_header(d, n, &hd, msg, cap);
    if (rc) return rc;
    if (hd.total_blocks > (1 << 20)) return lwp::JPEG_CAPACITY;          // a changed size field: do not follow it into gigabytes
    coef.resize((size_t)hd.total_blocks * 64);
    return lwp::jpeg_decode_blocks(d, n, &hd, coef.data(), coef.size(), qt, msg, cap);
}

int main(int argc, char** argv) {
    bool mutate = false;
    long ok = 0, refused = 0;
    std::vector<int16_t> coef;
    char msg[256];
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--mutate")) { mutate = true; continue; }
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<unsigned char> file;
        unsigned char chunk[4096];
        for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
        fclose(f);
        {
            std::unique_ptr<unsigned char[]> p(new unsigned char[file.size()]);
            memcpy(p.get(), file.data(), file.size());
            if (decode(p.get(), file.size(), coef, msg, sizeof msg) != lwp::JPEG_OK) { fprintf(stderr, "%s: %s\n", argv[a], msg); return 1; }
        }
        for (size_t n = 0; n < file.size(); ++n) {
            std::unique_ptr<unsigned char[]> p(new unsigned char[n ? n : 1]);
            memcpy(p.get(), file.data(), n);
            (decode(p.get(), n, coef, msg, sizeof msg) == lwp::JPEG_OK ? ok : refused)++;
        }
        if (!mutate) continue;
        std::unique_ptr<unsigned char[]> p(new unsigned char[file.size()]);
        memcpy(p.get(), file.data(), file.size());
        for (size_t i = 0; i < file.size(); ++i) {
            for (int v = 1; v < 256; ++v) {
                p[i] = (unsigned char)(file[i] ^ v);
                (decode(p.get(), file.size(), coef, msg, sizeof msg) == lwp::JPEG_OK ? ok : refused)++;
            }
            p[i] = file[i];
        }
    }
    printf("jpeg_host_check: %ld inputs decoded, %ld refused\n", ok, refused);
    return 0;
}
