// Stand-alone check of the JPEG batch plans (csrc/jpeg_batch.cpp): where every region of a batch's workspace lies and what the
// records say, which the kernels trust without a bounds check.  Meant to be built with the host compiler and
// -fsanitize=address,undefined (tests/test_jpeg_plan_host.py does): no HIP, no GPU, nothing loaded into another process.
//
//     jpeg_plan_check FILE...
//
// Decode, in host and in device entropy form: every FILE alone, all in one batch, the batch reversed, and the batch with a
// refused file in the middle (the host form must name it; the tolerant device form carries it as a file of no components).
// Encode needs no files: seven sizes in the three samplings with restart intervals 0, 1 and mcus_x, host and device frames,
// alone and as one mixed batch.  Every staging is a heap block of exactly the plan's upload bytes and every host frame one of
// exactly its pixels, so a fill that leaves either is an error the sanitizer sees.  For every plan: the regions lie in the
// documented order, disjoint and aligned (16 bytes; 256 for host frames, device-only regions, upload and total); every
// region a record names lies inside the workspace, behind the upload where the kernels write it, and overlaps no other
// record's; the start arrays do not decrease and end in the totals, which equal the sums over the headers or geometries.  The
// first violated property ends the program with status 1 and names the case.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../lightweight-human-pose-estimation.pytorch_amd/csrc/jpeg_batch.h"

using namespace lwp;

static std::string g_case;
static long g_plans = 0, g_records = 0;

[[noreturn]] static void violated(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "jpeg_plan_check: %s: ", g_case.c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define NEED(cond, ...) do { if (!(cond)) violated(__VA_ARGS__); } while (0)

// an address the plans must hand on without reading it: a caller's pixels, a device frame, the device workspace
static unsigned char* opaque(size_t v) { return reinterpret_cast<unsigned char*>((uintptr_t)0x100000000000 + v); }

struct Region { const char* name; size_t off, bytes, align; bool device_only; };
struct Span { size_t off, bytes; };

// the regions in their documented order
static void check_regions(const std::vector<Region>& r, size_t upload, size_t total) {
    NEED(upload % 256 == 0 && total % 256 == 0 && upload <= total, "upload %zu / total %zu is no multiple of 256", upload, total);
    size_t end = 0;
    for (const Region& x : r) {
        NEED(x.off % x.align == 0, "%s at %zu is not %zu-byte aligned", x.name, x.off, x.align);
        NEED(x.off >= end, "%s at %zu starts inside the region in front of it, which ends at %zu", x.name, x.off, end);
        end = x.off + x.bytes;
        NEED(x.device_only ? x.off >= upload : end <= upload, "%s [%zu, %zu) is on the wrong side of the upload's end %zu", x.name, x.off, end, upload);
    }
    NEED(end <= total, "the last region ends at %zu, the workspace at %zu", end, total);
    ++g_plans;
}

// what records of one kind name: inside [lo, hi), no two overlapping
static void check_spans(const char* what, std::vector<Span> s, size_t lo, size_t hi) {
    g_records += (long)s.size();
    std::sort(s.begin(), s.end(), [](const Span& a, const Span& b) { return a.off < b.off || (a.off == b.off && a.bytes < b.bytes); });
    size_t end = lo;
    for (const Span& x : s) {
        NEED(x.off >= lo && x.off + x.bytes <= hi, "%s [%zu, %zu) leaves [%zu, %zu)", what, x.off, x.off + x.bytes, lo, hi);
        NEED(x.off >= end || x.bytes == 0, "%s [%zu, %zu) overlaps the one in front of it, which ends at %zu", what, x.off, x.off + x.bytes, end);
        end = std::max(end, x.off + x.bytes);
    }
}

static void check_starts(const char* what, const unsigned* a, size_t n, uint64_t total) {
    for (size_t i = 0; i < n; ++i) NEED(a[i] <= a[i + 1], "%s [%zu] = %u decreases to %u", what, i, a[i], a[i + 1]);
    NEED(a[0] == 0 && a[n] == total, "%s runs from %u to %u, the total is %llu", what, a[0], a[n], (unsigned long long)total);
}

struct File { std::unique_ptr<unsigned char[]> p; size_t n = 0; };
struct Batch {
    std::vector<const unsigned char*> data;
    std::vector<size_t> len;
    std::vector<unsigned char*> out;                   // opaque to the plans: never dereferenced
    int bad = -1;                                      // the refused file, if one is in it
};

// the plane and image records of either decode form
static void check_decode_records(const JpegHeaders& H, const JpegDecodePlan& P, const Batch& B, const unsigned char* host) {
    const size_t N = H.hd.size();
    const JpegPlane* planes = reinterpret_cast<const JpegPlane*>(host + P.planes);
    const JpegImage* images = reinterpret_cast<const JpegImage*>(host + P.images);
    uint64_t blocks = 0, units = 0;
    std::vector<Span> of_planes, of_images;
    int p = 0;
    for (size_t i = 0; i < N; ++i) {
        const lwp_jpeg_header& f = H.hd[i];
        const JpegImage& im = images[i];
        NEED(im.out == B.out[i] && im.width == f.width && im.height == f.height && im.unit0 == units, "image record %zu is not its file's", i);
        for (int c = 0; c < f.components; ++c, ++p) {
            const size_t bytes = (size_t)f.blocks_w[c] * f.blocks_h[c] * 64;
            NEED(planes[p].block0 == blocks && planes[p].blocks_w == f.blocks_w[c], "plane record %d is not its component's", p);
            NEED(planes[p].qt + 64 <= N * kJpegQuantSlots * 64, "plane record %d: table offset %u leaves the tables", p, planes[p].qt);
            NEED(im.plane[c] == planes[p].plane && im.stride[c] == f.blocks_w[c] * 8, "image record %zu, plane %d differs from plane record %d", i, c, p);
            of_planes.push_back({(size_t)planes[p].plane, bytes});
            of_images.push_back({(size_t)im.plane[c], (size_t)im.stride[c] * f.blocks_h[c] * 8});
            blocks += (uint64_t)f.blocks_w[c] * f.blocks_h[c];
        }
        units += (uint64_t)f.height * (uint64_t)((f.width + kJpegPixelsPerThread - 1) / kJpegPixelsPerThread);
    }
    NEED(p == H.n_planes && blocks == H.blocks && units == H.units, "the totals are not the sums over the headers");
    check_spans("JpegPlane::plane", of_planes, P.plane_base, P.total);
    check_spans("JpegImage::plane", of_images, P.plane_base, P.total);
    check_starts("plane starts", reinterpret_cast<const unsigned*>(host + P.pstart), (size_t)H.n_planes, H.blocks);
    check_starts("image starts", reinterpret_cast<const unsigned*>(host + P.istart), N, H.units);
}

static std::vector<Region> decode_tail(const JpegHeaders& H, const JpegDecodePlan& P) {
    const size_t N = H.hd.size(), np = (size_t)H.n_planes;
    return {{"plane records", P.planes, np * sizeof(JpegPlane), 16, false}, {"plane starts", P.pstart, (np + 1) * 4, 16, false},
            {"image records", P.images, N * sizeof(JpegImage), 16, false}, {"image starts", P.istart, (N + 1) * 4, 16, false}};
}

static void decode_host_form(const Batch& B) {
    const int N = (int)B.data.size();
    char msg[kJpegMsg] = {0};
    JpegHeaders H;
    const int rc = jpeg_batch_headers(N, B.data.data(), B.len.data(), B.out.data(), false, &H, msg);
    if (B.bad >= 0) {
        char name[32];
        snprintf(name, sizeof name, "image %d: ", B.bad);
        NEED(rc == JPEG_REFUSED && H.refused == B.bad && !strncmp(msg, name, strlen(name)), "the refused file %d is not the one named: \"%s\"", B.bad, msg);
        return;
    }
    NEED(rc == JPEG_OK, "the header pass refuses the batch: %s", msg);
    JpegDecodePlan P;
    jpeg_decode_plan(H, &P);
    std::vector<Region> r = {{"coefficients", P.coef, (size_t)H.blocks * 128, 16, false},
                             {"quantisation tables", P.qt, (size_t)N * kJpegQuantSlots * 128, 16, false}};
    for (const Region& x : decode_tail(H, P)) r.push_back(x);
    r.push_back({"component planes", P.plane_base, (size_t)H.blocks * 64, 256, true});
    check_regions(r, P.upload, P.total);
    std::unique_ptr<unsigned char[]> host(new unsigned char[P.upload]);
    jpeg_decode_fill(H, P, B.out.data(), host.get());
    check_decode_records(H, P, B, host.get());
}

static void decode_device_form(const Batch& B) {
    const int N = (int)B.data.size();
    char msg[kJpegMsg] = {0};
    JpegHeaders H;
    JpegEntropyPlan P;
    NEED(jpeg_batch_headers(N, B.data.data(), B.len.data(), B.out.data(), B.bad >= 0, &H, msg) == JPEG_OK, "the header pass refuses the batch: %s", msg);
    NEED(H.refused == B.bad && (B.bad < 0 || (H.verdict[B.bad] && !H.hd[B.bad].components)), "the refused file %d is not the one found (%d)", B.bad, H.refused);
    NEED(jpeg_entropy_plan(H, B.len.data(), &P, msg) == JPEG_OK, "the plan refuses the batch: %s", msg);
    std::unique_ptr<unsigned char[]> host(new unsigned char[P.d.upload]);
    std::vector<JpegScanSeg> scan((size_t)P.seg_at[N] + 1);
    std::vector<size_t> n_scan((size_t)N, 0);
    JpegHuffFlat* tables = reinterpret_cast<JpegHuffFlat*>(host.get() + P.tab);
    uint16_t* qt = reinterpret_cast<uint16_t*>(host.get() + P.d.qt);
    uint64_t subs_of_4 = 0;
    for (int i = 0; i < N; ++i) {                      // the pre-pass, into the staging as the library runs it
        if (H.verdict[i]) continue;
        size_t nb = 0;
        const int rc = jpeg_scan_segments(B.data[i], B.len[i], &H.hd[i], host.get() + P.bytes + P.byte_at[i], (size_t)(P.byte_at[i + 1] - P.byte_at[i]), &nb,
                                          scan.data() + P.seg_at[i], (size_t)(P.seg_at[i + 1] - P.seg_at[i]), &n_scan[i],
                                          tables + (size_t)i * kJpegHuffPerFile, qt + (size_t)i * kJpegQuantSlots * 64);
        NEED(rc == JPEG_OK && n_scan[i] == jpeg_expected_segments(H.hd[i]), "the pre-pass refuses file %d", i);
        for (size_t k = 0; k < n_scan[i]; ++k) subs_of_4 += std::max<uint64_t>(1, ((uint64_t)scan[P.seg_at[i] + k].n_bytes + 3) / 4);
    }
    // the fewest and the most subsequences subseq_bytes allows: one a segment, and one every four bytes
    for (int subseq : {1 << 30, 4}) {
        NEED(jpeg_entropy_fill(H, &P, scan.data(), n_scan.data(), subseq, host.get(), msg) == JPEG_OK, "the fill refuses the batch: %s", msg);
        NEED(P.n_segs == P.seg_at[N] && P.n_subs == (subseq == 4 ? subs_of_4 : P.n_segs), "%u segments, %u subsequences at %d bytes each", P.n_segs, P.n_subs, subseq);
        jpeg_entropy_place(H, &P);
        jpeg_decode_fill(H, P.d, B.out.data(), host.get());
        std::vector<Region> r = {{"un-stuffed scans", P.bytes, (size_t)P.byte_at[N] + 8, 16, false},
                                 {"Huffman tables", P.tab, (size_t)N * kJpegHuffPerFile * sizeof(JpegHuffFlat), 16, false},
                                 {"quantisation tables", P.d.qt, (size_t)N * kJpegQuantSlots * 128, 16, false},
                                 {"file records", P.files, (size_t)N * sizeof(JpegEntFile), 16, false},
                                 {"file workgroup starts", P.fwg, ((size_t)N + 1) * 4, 16, false},
                                 {"segment records", P.segs, (size_t)P.n_segs * sizeof(JpegEntSeg), 16, false},
                                 {"segment subsequence starts", P.ssub, ((size_t)P.n_segs + 1) * 4, 16, false}};
        for (const Region& x : decode_tail(H, P.d)) r.push_back(x);
        r.push_back({"coefficients", P.d.coef, (size_t)H.blocks * 128, 256, true});
        r.push_back({"status words", P.status, ((size_t)N + 2) * 4, 4, true});
        r.push_back({"subsequence records", P.rec, (size_t)P.n_subs * 8, 256, true});
        r.push_back({"positions", P.subpos, (size_t)P.n_subs * 4, 256, true});
        r.push_back({"workgroup entries", P.wg_entry, (size_t)P.n_wgs * 8, 256, true});
        r.push_back({"workgroup flags", P.wg_dirty, (size_t)P.n_wgs * 4, 256, true});
        r.push_back({"component planes", P.d.plane_base, (size_t)H.blocks * 64, 256, true});
        check_regions(r, P.d.upload, P.d.total);
        NEED(P.status == P.d.coef + (size_t)H.blocks * 128, "the status words do not follow the coefficients: one memset clears both");
        NEED(P.stage_bytes >= P.d.upload + ((size_t)N + 2) * 4, "the staging has no room for the status words");
        check_decode_records(H, P.d, B, host.get());
        const JpegEntFile* files = reinterpret_cast<const JpegEntFile*>(host.get() + P.files);
        const JpegEntSeg* segs = reinterpret_cast<const JpegEntSeg*>(host.get() + P.segs);
        std::vector<Span> of_segs, of_files;
        uint64_t wgs = 0;
        for (unsigned s = 0; s < P.n_segs; ++s) {
            NEED(segs[s].file < (unsigned)N && s >= files[segs[s].file].seg0 && s - files[segs[s].file].seg0 < files[segs[s].file].n_segs, "segment %u is not its file's", s);
            of_segs.push_back({P.bytes + segs[s].byte0, segs[s].n_bytes});
        }
        for (int i = 0; i < N; ++i) {
            of_files.push_back({P.d.coef + (size_t)files[i].block0 * 128, (size_t)files[i].total_blocks * 128});
            NEED(files[i].total_blocks == (unsigned)H.hd[i].total_blocks && files[i].wg0 == wgs, "file record %d is not its file's", i);
            NEED(files[i].n_wgs == (files[i].n_subs + kJpegEntropyGroup - 1) / kJpegEntropyGroup, "file record %d: %u workgroups for %u subsequences", i, files[i].n_wgs, files[i].n_subs);
            wgs += files[i].n_wgs;
        }
        check_spans("JpegEntSeg::byte0", of_segs, P.bytes, P.bytes + (size_t)P.byte_at[N]);
        check_spans("JpegEntFile::block0", of_files, P.d.coef, P.status);
        check_starts("file workgroup starts", reinterpret_cast<const unsigned*>(host.get() + P.fwg), (size_t)N, P.n_wgs);
        check_starts("segment subsequence starts", reinterpret_cast<const unsigned*>(host.get() + P.ssub), P.n_segs, P.n_subs);
        NEED(wgs == P.n_wgs, "the workgroups of the files sum to %llu, the plan has %u", (unsigned long long)wgs, P.n_wgs);
    }
}

static void decode_case(const char* what, const std::vector<File>& files, const std::vector<int>& order, int bad_at = -1) {
    static const unsigned char junk[4] = {'n', 'o', 'p', 'e'};
    Batch B;
    for (size_t k = 0; k < order.size(); ++k) {
        if ((int)k == bad_at) { B.bad = (int)B.data.size(); B.data.push_back(junk); B.len.push_back(sizeof junk); B.out.push_back(opaque(1 << 20)); }
        B.data.push_back(files[order[k]].p.get()); B.len.push_back(files[order[k]].n); B.out.push_back(opaque(4096 * (size_t)(order[k] + 1)));
    }
    g_case = std::string(what) + ", host entropy";
    decode_host_form(B);
    g_case = std::string(what) + ", device entropy";
    decode_device_form(B);
}

static void encode_case(const std::vector<std::pair<int, int>>& sizes, int subsampling, int restart_interval, bool mem_host) {
    const int N = (int)sizes.size();
    char name[160];
    snprintf(name, sizeof name, "encode %d x %d%s, sampling %d, restart interval %d, %s frames", sizes[0].first, sizes[0].second, N > 1 ? " and others" : "",
             subsampling, restart_interval, mem_host ? "host" : "device");
    g_case = name;
    std::vector<std::unique_ptr<unsigned char[]>> pixels;
    std::vector<const unsigned char*> frames;
    std::vector<int> heights, widths;
    for (int i = 0; i < N; ++i) {
        heights.push_back(sizes[i].first); widths.push_back(sizes[i].second);
        const size_t n = (size_t)heights[i] * widths[i] * 3;
        pixels.emplace_back(new unsigned char[n]);
        memset(pixels.back().get(), i + 1, n);
        frames.push_back(mem_host ? pixels.back().get() : opaque(4096 * (size_t)(i + 1)));     // a device frame
    }
    char msg[kJpegMsg] = {0};
    JpegEncPlan P;
    NEED(jpeg_enc_plan(N, frames.data(), mem_host, heights.data(), widths.data(), subsampling, restart_interval, &P, msg) == JPEG_OK, "the plan refuses: %s", msg);
    uint64_t blocks = 0, chunks = 0, intervals = 0;
    for (const JpegEncGeom& g : P.geom) {
        blocks += (uint64_t)g.total_blocks; intervals += (uint64_t)g.intervals;
        chunks += (jpeg_enc_unstuffed_bound(g) + kJpegEncChunk - 1) / kJpegEncChunk;
    }
    NEED(blocks == P.blocks && chunks == P.chunks, "the totals are not the sums over the geometries");
    std::vector<Region> r = {{"image records", P.images, (size_t)N * sizeof(JpegEncImage), 16, false}, {"block starts", P.bstart, ((size_t)N + 1) * 4, 16, false},
                             {"chunk starts", P.cstart, ((size_t)N + 1) * 4, 16, false}, {"quantisation tables", P.qt, 2 * 64 * 2, 16, false},
                             {"Huffman codes", P.huff, sizeof(JpegEncHuff), 16, false}};
    if (mem_host)
        for (int i = 0; i < N; ++i) r.push_back({"host frame", P.frame[i], (size_t)heights[i] * widths[i] * 3, 256, false});
    r.push_back({"coefficients", P.coef, (size_t)blocks * 128, 256, true});
    r.push_back({"bit counts", P.bits, (size_t)blocks * 4, 256, true});
    r.push_back({"bit offsets", P.offs, (size_t)blocks * 4, 256, true});
    r.push_back({"interval starts", P.istart, (size_t)intervals * 4, 256, true});
    r.push_back({"un-stuffed lengths", P.ulen, (size_t)N * 4, 256, true});
    r.push_back({"stuffed lengths", P.slen, (size_t)N * 4, 256, true});
    r.push_back({"chunk counts", P.ffbase, (size_t)chunks * 4, 256, true});
    r.push_back({"un-stuffed scans", P.ubytes, P.ubytes_total, 256, true});
    for (int i = 0; i < N; ++i) r.push_back({"stuffed scan", P.sbytes[i], jpeg_enc_scan_bound(P.geom[i]), 16, true});
    check_regions(r, P.upload, P.total);
    NEED(P.ubytes_total == (size_t)chunks * kJpegEncChunk, "the un-stuffed scans take %zu bytes for %llu chunks", P.ubytes_total, (unsigned long long)chunks);
    std::unique_ptr<unsigned char[]> host(new unsigned char[P.upload]);
    const unsigned char* dev = opaque((size_t)1 << 40);                         // the workspace's device address
    jpeg_enc_fill(P, frames.data(), mem_host, heights.data(), widths.data(), 75, dev, host.get());
    const JpegEncImage* images = reinterpret_cast<const JpegEncImage*>(host.get() + P.images);
    std::vector<Span> u, s, f;
    uint64_t i0 = 0;
    for (int i = 0; i < N; ++i) {
        const JpegEncImage& im = images[i];
        NEED(im.width == widths[i] && im.height == heights[i] && im.n_blocks == (unsigned)P.geom[i].total_blocks && im.int0 == i0, "image record %d is not its image's", i);
        NEED(im.ubytes % 16 == 0 && im.ucap == im.n_chunks * (unsigned)kJpegEncChunk && im.sbytes == (long long)P.sbytes[i], "image record %d: its scans are not the plan's", i);
        u.push_back({(size_t)im.ubytes, im.ucap});
        s.push_back({(size_t)im.sbytes, im.scap});
        if (mem_host) {
            f.push_back({(size_t)((uintptr_t)im.src - (uintptr_t)dev), (size_t)heights[i] * widths[i] * 3});
            NEED(!memcmp(host.get() + P.frame[i], frames[i], f.back().bytes), "host frame %d is not in its slot", i);
        } else {
            NEED(im.src == frames[i], "image record %d does not hold its device frame", i);
        }
        i0 += im.n_int;
    }
    NEED(i0 == intervals, "the intervals of the records sum to %llu, the geometries' to %llu", (unsigned long long)i0, (unsigned long long)intervals);
    check_spans("JpegEncImage::ubytes", u, P.ubytes, P.ubytes + P.ubytes_total);
    check_spans("JpegEncImage::sbytes", s, P.ubytes + P.ubytes_total, P.total);
    check_spans("host-frame slot", f, P.huff + sizeof(JpegEncHuff), P.upload);
    check_starts("block starts", reinterpret_cast<const unsigned*>(host.get() + P.bstart), (size_t)N, blocks);
    check_starts("chunk starts", reinterpret_cast<const unsigned*>(host.get() + P.cstart), (size_t)N, chunks);
}

int main(int argc, char** argv) {
    std::vector<File> files;
    for (int a = 1; a < argc; ++a) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<unsigned char> all;
        unsigned char chunk[4096];
        for (size_t n; (n = fread(chunk, 1, sizeof chunk, fp)) > 0;) all.insert(all.end(), chunk, chunk + n);
        fclose(fp);
        File f;
        f.n = all.size();
        f.p.reset(new unsigned char[f.n ? f.n : 1]);   // exactly its length: a read past its end is the sanitizer's to see
        memcpy(f.p.get(), all.data(), f.n);
        files.push_back(std::move(f));
    }
    if (files.empty()) { fprintf(stderr, "usage: jpeg_plan_check FILE...\n"); return 2; }
    std::vector<int> all;
    for (int i = 0; i < (int)files.size(); ++i) {
        decode_case(argv[i + 1], files, {i});
        all.push_back(i);
    }
    decode_case("all files", files, all);
    decode_case("all files with a refused one in the middle", files, all, (int)all.size() / 2);
    std::reverse(all.begin(), all.end());
    decode_case("all files reversed", files, all);

    const std::vector<std::pair<int, int>> sizes = {{1, 1}, {7, 7}, {8, 9}, {16, 32}, {17, 23}, {31, 65}, {100, 75}};
    for (int sub = 0; sub < 3; ++sub)
        for (bool mem_host : {true, false}) {
            int widest = 1;
            for (const auto& hw : sizes) {
                JpegEncGeom g;
                NEED(jpeg_enc_geometry(hw.first, hw.second, sub, 0, &g), "no geometry for %d x %d", hw.first, hw.second);
                widest = std::max(widest, g.mcus_x);
                for (int ri : {0, 1, g.mcus_x}) encode_case({hw}, sub, ri, mem_host);
            }
            for (int ri : {0, 1, widest}) encode_case(sizes, sub, ri, mem_host);
        }
    printf("jpeg_plan_check: %ld plans of %d files and %zu sizes hold, %ld regions named by records inside them\n", g_plans, argc - 1, sizes.size(), g_records);
    return 0;
}
