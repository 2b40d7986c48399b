// Stand-alone robustness walk of the host pre-pass of the device entropy decoder (jpeg_scan_segments in csrc/jpeg_host.cpp),
// meant to be built with the host compiler and -fsanitize=address,undefined (tests/test_jpeg_entropy_host.py does): no HIP, no
// GPU, nothing loaded into another process.
//
//     jpeg_scan_check FILE... [--mutate FILE...]
//
// Every FILE must pass the pre-pass; then every proper prefix of it is walked, and for the files behind --mutate every
// single-bit flip and every single-byte change of the bytes from the scan's first to the end.  Each input lives in a heap block
// of exactly its length, and the outputs in blocks of exactly the sizes the header comments promise to suffice, so a read or
// write past an end is an error the sanitizer sees.  The pre-pass may refuse what the host decoder refuses and nothing else:
// a file it refuses and jpeg_decode_blocks accepts ends the program with status 1.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../lightweight-human-pose-estimation.pytorch_amd/csrc/jpeg_host.h"

static long g_ok = 0, g_refused = 0, g_disagree = 0;

// JPEG_OK / JPEG_REFUSED of the pre-pass; -1: the header itself is refused (the pre-pass is not called)
static int scan(const unsigned char* d, size_t n) {
    lwp_jpeg_header hd;
    if (lwp::jpeg_parse_header(d, n, &hd, nullptr, 0) != lwp::JPEG_OK) return -1;
    if (hd.total_blocks > (1 << 20)) return -1;                            // a changed size field: do not follow it into gigabytes
    const size_t n_segs = lwp::jpeg_expected_segments(hd);
    std::unique_ptr<unsigned char[]> bytes(new unsigned char[n ? n : 1]);
    std::unique_ptr<lwp::JpegScanSeg[]> segs(new lwp::JpegScanSeg[n_segs]);
    std::unique_ptr<lwp::JpegHuffFlat[]> tables(new lwp::JpegHuffFlat[lwp::kJpegHuffPerFile]);
    std::unique_ptr<uint16_t[]> qt(new uint16_t[4 * 64]);
    size_t nb = 0, ns = 0;
    const int rc = lwp::jpeg_scan_segments(d, n, &hd, bytes.get(), n, &nb, segs.get(), n_segs, &ns, tables.get(), qt.get());
    if (rc == lwp::JPEG_OK) {
        size_t at = 0;
        for (size_t s = 0; s < ns; ++s) {                                  // the segments tile the un-stuffed bytes
            if (segs[s].byte0 != at) { ++g_disagree; fprintf(stderr, "segment %zu starts at %u, not %zu\n", s, segs[s].byte0, at); }
            at += segs[s].n_bytes;
        }
        if (at != nb || ns != n_segs) { ++g_disagree; fprintf(stderr, "%zu bytes in %zu segments, %zu and %zu expected\n", at, ns, nb, n_segs); }
    } else {
        std::vector<int16_t> coef((size_t)hd.total_blocks * 64);
        lwp_jpeg_header now;
        if (lwp::jpeg_decode_blocks(d, n, &now, coef.data(), coef.size(), qt.get(), nullptr, 0) == lwp::JPEG_OK) {
            ++g_disagree;
            fprintf(stderr, "the pre-pass refuses an input of %zu bytes that the host decoder accepts\n", n);
        }
    }
    (rc == lwp::JPEG_OK ? g_ok : g_refused)++;
    return rc;
}

int main(int argc, char** argv) {
    bool mutate = false;
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
            if (scan(p.get(), file.size()) != lwp::JPEG_OK) { fprintf(stderr, "%s: refused\n", argv[a]); return 1; }
        }
        for (size_t n = 0; n < file.size(); ++n) {
            std::unique_ptr<unsigned char[]> p(new unsigned char[n ? n : 1]);
            memcpy(p.get(), file.data(), n);
            scan(p.get(), n);
        }
        if (!mutate) continue;
        size_t from = 0;                                                   // the first SOS: the scan starts behind it
        for (size_t i = 0; i + 1 < file.size(); ++i)
            if (file[i] == 0xFF && file[i + 1] == 0xDA) { from = i; break; }
        std::unique_ptr<unsigned char[]> p(new unsigned char[file.size()]);
        memcpy(p.get(), file.data(), file.size());
        for (size_t i = from; i < file.size(); ++i) {
            for (int v = 1; v < 256; ++v) {
                p[i] = (unsigned char)(file[i] ^ v);
                scan(p.get(), file.size());
            }
            p[i] = file[i];
        }
    }
    printf("jpeg_scan_check: %ld inputs accepted so far, %ld refused, %ld disagreements\n", g_ok, g_refused, g_disagree);
    return g_disagree ? 1 : 0;
}
