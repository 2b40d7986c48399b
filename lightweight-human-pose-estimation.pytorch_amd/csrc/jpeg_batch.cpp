// The host arithmetic of a JPEG batch: see jpeg_batch.h.  No HIP include.
#include "jpeg_batch.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace lwp {

static uint64_t pixel_groups(const lwp_jpeg_header& f) {
    return (uint64_t)f.height * (uint64_t)((f.width + kJpegPixelsPerThread - 1) / kJpegPixelsPerThread);
}

int jpeg_batch_headers(int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out, bool tolerant,
                       JpegHeaders* H, char* msg) {
    char why[256];
    H->hd.assign((size_t)N, lwp_jpeg_header{});
    H->verdict.assign((size_t)N, JPEG_OK);
    for (int i = 0; i < N; ++i) {
        lwp_jpeg_header& f = H->hd[i];
        if (!data[i] || (out && !out[i])) { snprintf(msg, kJpegMsg, "image %d: data / out is null", i); return JPEG_REFUSED; }
        why[0] = 0;
        if (jpeg_parse_header(data[i], len[i], &f, why, sizeof why) != JPEG_OK) {
            if (H->refused < 0) { H->refused = i; snprintf(msg, kJpegMsg, "image %d: %s", i, why); }
            if (!tolerant) return JPEG_REFUSED;
            f = lwp_jpeg_header{};
            f.h_samp[0] = f.v_samp[0] = 1;
            H->verdict[i] = JPEG_REFUSED;
        }
        H->blocks += (uint64_t)f.total_blocks;
        H->units += pixel_groups(f);
        H->n_planes += f.components;
        H->in_bytes += len[i];
    }
    if (H->blocks <= 0x7fffffffu && H->units <= 0x7fffffffu) return JPEG_OK;
    snprintf(msg, kJpegMsg, "the batch has 2^31 or more blocks or pixel groups: decode it in parts");
    return JPEG_CAPACITY;
}

// the four regions both decode forms end their upload with, and the end of the upload
static void decode_records(const JpegHeaders& H, Layout& L, JpegDecodePlan* P) {
    const size_t N = H.hd.size();
    P->planes = L.take<JpegPlane>((size_t)H.n_planes); P->pstart = L.take<unsigned>((size_t)H.n_planes + 1);
    P->images = L.take<JpegImage>(N); P->istart = L.take<unsigned>(N + 1);
    P->upload = L.align(256);
}

void jpeg_decode_plan(const JpegHeaders& H, JpegDecodePlan* P) {
    Layout L;
    P->coef = L.take<int16_t>((size_t)H.blocks * 64); P->qt = L.take<uint16_t>(H.hd.size() * kJpegQuantSlots * 64);
    decode_records(H, L, P);
    P->plane_base = L.take<unsigned char>((size_t)H.blocks * 64, 256);
    P->total = L.align(256);
}

void jpeg_decode_fill(const JpegHeaders& H, const JpegDecodePlan& P, unsigned char* const* out, unsigned char* host) {
    JpegPlane* planes = reinterpret_cast<JpegPlane*>(host + P.planes);
    unsigned* pstart = reinterpret_cast<unsigned*>(host + P.pstart);
    JpegImage* images = reinterpret_cast<JpegImage*>(host + P.images);
    unsigned* istart = reinterpret_cast<unsigned*>(host + P.istart);
    const int N = (int)H.hd.size();
    uint64_t b0 = 0, u0 = 0;
    int p = 0;
    for (int i = 0; i < N; ++i) {                      // a file of no components takes no plane record
        const lwp_jpeg_header& f = H.hd[i];
        JpegImage& im = images[i];
        memset(&im, 0, sizeof im);
        im.unit0 = (unsigned)u0; istart[i] = (unsigned)u0;
        im.width = f.width; im.height = f.height;
        im.mode = f.components == 1 ? 0 : f.h_samp[0] == 1 ? 1 : f.v_samp[0] == 1 ? 2 : 3;
        im.chroma_w = f.components == 1 ? 0 : (f.width + f.h_samp[0] - 1) / f.h_samp[0];
        im.chroma_h = f.components == 1 ? 0 : (f.height + f.v_samp[0] - 1) / f.v_samp[0];
        im.out = out ? out[i] : nullptr;
        for (int c = 0; c < f.components; ++c) {
            JpegPlane& pl = planes[p];
            pl.block0 = (unsigned)b0; pstart[p] = (unsigned)b0;
            pl.blocks_w = f.blocks_w[c];
            pl.qt = (unsigned)(((size_t)i * kJpegQuantSlots + (size_t)f.quant_table[c]) * 64);
            pl.pad_ = 0;
            pl.plane = (long long)(P.plane_base + b0 * 64);
            im.plane[c] = pl.plane; im.stride[c] = f.blocks_w[c] * 8;
            b0 += (uint64_t)f.blocks_w[c] * f.blocks_h[c];
            ++p;
        }
        u0 += pixel_groups(f);
    }
    pstart[p] = (unsigned)b0; istart[N] = (unsigned)u0;
}

int jpeg_entropy_plan(const JpegHeaders& H, const size_t* len, JpegEntropyPlan* P, char* msg) {
    const size_t N = H.hd.size();
    P->seg_at.assign(N + 1, 0); P->byte_at.assign(N + 1, 0);
    for (size_t i = 0; i < N; ++i) {
        P->seg_at[i + 1] = P->seg_at[i] + (H.verdict[i] ? 0 : (uint64_t)jpeg_expected_segments(H.hd[i]));
        P->byte_at[i + 1] = P->byte_at[i] + (H.verdict[i] ? 0 : (((uint64_t)len[i] + 3) & ~(uint64_t)3) + 8);
    }
    const uint64_t seg_cap = P->seg_at[N], byte_cap = P->byte_at[N];
    if (byte_cap > 0xfffffff0u || seg_cap > 0x7fffffffu) {
        snprintf(msg, kJpegMsg, "the batch has 2^32 or more bytes or 2^31 or more restart intervals: decode it in parts");
        return JPEG_CAPACITY;
    }
    Layout L;
    P->bytes = L.take<unsigned char>((size_t)byte_cap + 8); P->tab = L.take<JpegHuffFlat>(N * kJpegHuffPerFile);
    P->d.qt = L.take<uint16_t>(N * kJpegQuantSlots * 64);
    P->files = L.take<JpegEntFile>(N); P->fwg = L.take<unsigned>(N + 1);
    P->segs = L.take<JpegEntSeg>((size_t)seg_cap); P->ssub = L.take<unsigned>((size_t)seg_cap + 1);
    decode_records(H, L, &P->d);
    P->stage_bytes = P->d.upload + (N + 2) * 4;
    return JPEG_OK;
}

int jpeg_entropy_fill(const JpegHeaders& H, JpegEntropyPlan* P, const JpegScanSeg* scan, const size_t* n_scan, int subseq,
                      unsigned char* host, char* msg) {
    JpegEntFile* files = reinterpret_cast<JpegEntFile*>(host + P->files);
    unsigned* fwg = reinterpret_cast<unsigned*>(host + P->fwg);
    JpegEntSeg* segs = reinterpret_cast<JpegEntSeg*>(host + P->segs);
    unsigned* ssub = reinterpret_cast<unsigned*>(host + P->ssub);
    const int N = (int)H.hd.size();
    uint64_t n_subs = 0, n_wgs = 0, b0 = 0;
    size_t n_segs = 0;
    for (int i = 0; i < N; ++i) {
        const lwp_jpeg_header& f = H.hd[i];
        JpegEntFile& ef = files[i];
        memset(&ef, 0, sizeof ef);
        fwg[i] = (unsigned)n_wgs;
        ef.seg0 = (unsigned)n_segs; ef.sub0 = (unsigned)n_subs; ef.wg0 = (unsigned)n_wgs;
        ef.block0 = (unsigned)b0; ef.total_blocks = (unsigned)f.total_blocks;
        ef.components = f.components; ef.mcus_x = std::max(f.mcus_x, 1);
        ef.h0 = std::max(f.h_samp[0], 1); ef.v0 = std::max(f.v_samp[0], 1);
        ef.blocks_per_mcu = f.components == 3 ? ef.h0 * ef.v0 + 2 : 1;
        unsigned pb = 0;
        for (int c = 0; c < f.components; ++c) { ef.plane_block[c] = pb; ef.blocks_w[c] = f.blocks_w[c]; pb += (unsigned)(f.blocks_w[c] * f.blocks_h[c]); }
        b0 += (uint64_t)f.total_blocks;
        if (H.verdict[i]) continue;
        for (size_t k = 0; k < n_scan[i]; ++k) {
            const JpegScanSeg& sc = scan[P->seg_at[i] + k];
            JpegEntSeg& sg = segs[n_segs];
            sg.byte0 = (unsigned)(P->byte_at[i] + sc.byte0); sg.n_bytes = sc.n_bytes;
            sg.first_block = sc.first_mcu * (unsigned)ef.blocks_per_mcu; sg.n_blocks = sc.n_mcus * (unsigned)ef.blocks_per_mcu;
            sg.sub0 = (unsigned)n_subs; sg.file = (unsigned)i;
            ssub[n_segs++] = (unsigned)n_subs;
            n_subs += std::max<uint64_t>(1, ((uint64_t)sc.n_bytes + (uint64_t)subseq - 1) / (uint64_t)subseq);
            if (n_subs > 0x7fffffffu) {
                snprintf(msg, kJpegMsg, "the batch has 2^31 or more subsequences: decode it in parts or with larger subsequences");
                return JPEG_CAPACITY;
            }
        }
        ef.n_segs = (unsigned)(n_segs - ef.seg0); ef.n_subs = (unsigned)(n_subs - ef.sub0);
        ef.n_wgs = (ef.n_subs + kJpegEntropyGroup - 1) / kJpegEntropyGroup;
        n_wgs += ef.n_wgs;
    }
    fwg[N] = (unsigned)n_wgs; ssub[n_segs] = (unsigned)n_subs;
    P->n_segs = (unsigned)n_segs; P->n_subs = (unsigned)n_subs; P->n_wgs = (unsigned)n_wgs;
    return JPEG_OK;
}

void jpeg_entropy_place(const JpegHeaders& H, JpegEntropyPlan* P) {
    Layout L;
    L.at = P->d.upload;
    P->d.coef = L.take<int16_t>((size_t)H.blocks * 64, 256);
    P->status = L.take<int>(H.hd.size() + 2, 4);       // right behind the coefficients: one memset clears both
    P->rec = L.take<uint64_t>(P->n_subs, 256); P->subpos = L.take<unsigned>(P->n_subs, 256);
    P->wg_entry = L.take<uint64_t>(P->n_wgs, 256); P->wg_dirty = L.take<unsigned>(P->n_wgs, 256);
    P->d.plane_base = L.take<unsigned char>((size_t)H.blocks * 64, 256);
    P->d.total = L.align(256);
}

int jpeg_enc_plan(int N, const unsigned char* const* frames, bool mem_host, const int* heights, const int* widths, int subsampling,
                  int restart_interval, JpegEncPlan* P, char* msg) {
    P->geom.assign((size_t)N, JpegEncGeom{});
    P->restart_interval = restart_interval;
    uint64_t intervals = 0, pixels = 0, scan_bytes = 0;
    for (int i = 0; i < N; ++i) {
        if (!frames[i]) { snprintf(msg, kJpegMsg, "image %d: the frame is null", i); return JPEG_REFUSED; }
        JpegEncGeom& g = P->geom[i];
        if (!jpeg_enc_geometry(heights[i], widths[i], subsampling, restart_interval, &g)) {
            snprintf(msg, kJpegMsg, "image %d: jpeg encode: %d x %d: height and width must be 1..65535", i, heights[i], widths[i]);
            return JPEG_REFUSED;
        }
        if ((uint64_t)g.total_blocks * kJpegEncBlockBytes * 8 >= ((uint64_t)1 << 32)) {       // bit offsets are 32-bit
            snprintf(msg, kJpegMsg, "image %d: jpeg encode: %d x %d has too many blocks for one scan: encode it in tiles", i, heights[i], widths[i]);
            return JPEG_CAPACITY;
        }
        P->blocks += (uint64_t)g.total_blocks;
        intervals += (uint64_t)g.intervals;
        P->chunks += (jpeg_enc_unstuffed_bound(g) + kJpegEncChunk - 1) / kJpegEncChunk;
        pixels += (uint64_t)heights[i] * (uint64_t)widths[i] * 3;
        scan_bytes += 3 * jpeg_enc_unstuffed_bound(g);
    }
    if (P->blocks > 0x7fffffffu || P->chunks > 0x7fffffffu || scan_bytes + P->blocks * 136 + pixels > ((uint64_t)1 << 36)) {
        snprintf(msg, kJpegMsg, "jpeg encode: the batch needs more than 64 GiB of workspace: encode it in parts");
        return JPEG_CAPACITY;
    }
    Layout L;
    P->images = L.take<JpegEncImage>((size_t)N); P->bstart = L.take<unsigned>((size_t)N + 1); P->cstart = L.take<unsigned>((size_t)N + 1);
    P->qt = L.take<uint16_t>(2 * 64); P->huff = L.take<JpegEncHuff>(1);
    P->frame.assign((size_t)N, 0);
    if (mem_host)
        for (int i = 0; i < N; ++i) P->frame[i] = L.take<unsigned char>((size_t)heights[i] * widths[i] * 3, 256);
    P->upload = L.align(256);
    P->coef = L.take<int16_t>((size_t)P->blocks * 64, 256);
    P->bits = L.take<unsigned>((size_t)P->blocks, 256); P->offs = L.take<unsigned>((size_t)P->blocks, 256);
    P->istart = L.take<unsigned>((size_t)intervals, 256);
    P->ulen = L.take<unsigned>((size_t)N, 256); P->slen = L.take<unsigned>((size_t)N, 256);
    P->ffbase = L.take<unsigned>((size_t)P->chunks, 256);
    P->ubytes = L.take<unsigned char>((size_t)P->chunks * kJpegEncChunk, 256);     // back to back, whole chunks each: one memset
    P->ubytes_total = (size_t)P->chunks * kJpegEncChunk;
    P->sbytes.assign((size_t)N, 0);
    for (int i = 0; i < N; ++i) P->sbytes[i] = L.take<unsigned char>(jpeg_enc_scan_bound(P->geom[i]));
    P->total = L.align(256);
    return JPEG_OK;
}

void jpeg_enc_fill(const JpegEncPlan& P, const unsigned char* const* frames, bool mem_host, const int* heights, const int* widths,
                   int quality, const unsigned char* dev, unsigned char* host) {
    JpegEncImage* images = reinterpret_cast<JpegEncImage*>(host + P.images);
    unsigned* bstart = reinterpret_cast<unsigned*>(host + P.bstart);
    unsigned* cstart = reinterpret_cast<unsigned*>(host + P.cstart);
    const int N = (int)P.geom.size();
    uint64_t b0 = 0, c0 = 0, i0 = 0;
    for (int i = 0; i < N; ++i) {
        const JpegEncGeom& g = P.geom[i];
        JpegEncImage& im = images[i];
        memset(&im, 0, sizeof im);
        const size_t n_chunks = (jpeg_enc_unstuffed_bound(g) + kJpegEncChunk - 1) / kJpegEncChunk;
        im.ubytes = (long long)(P.ubytes + c0 * kJpegEncChunk); im.ucap = (unsigned)(n_chunks * kJpegEncChunk);
        im.sbytes = (long long)P.sbytes[i]; im.scap = (unsigned)jpeg_enc_scan_bound(g);
        im.width = widths[i]; im.height = heights[i]; im.hs = g.hs; im.vs = g.vs; im.mcus_x = g.mcus_x; im.mcus_y = g.mcus_y;
        unsigned p0 = 0;
        for (int c = 0; c < 3; ++c) {
            im.blocks_w[c] = g.blocks_w[c]; im.real_w[c] = g.real_w[c]; im.real_h[c] = g.real_h[c];
            im.plane0[c] = p0;
            p0 += (unsigned)(g.blocks_w[c] * g.blocks_h[c]);
        }
        im.block0 = (unsigned)b0; im.n_blocks = (unsigned)g.total_blocks;
        im.per_mcu = (unsigned)(g.hs * g.vs + 2); im.ri_blocks = im.per_mcu * (unsigned)P.restart_interval;
        im.int0 = (unsigned)i0; im.n_int = (unsigned)g.intervals;
        im.chunk0 = (unsigned)c0; im.n_chunks = (unsigned)n_chunks;
        bstart[i] = (unsigned)b0; cstart[i] = (unsigned)c0;
        b0 += (uint64_t)g.total_blocks; c0 += n_chunks; i0 += (uint64_t)g.intervals;
        im.src = frames[i];
        if (mem_host) {
            memcpy(host + P.frame[i], frames[i], (size_t)heights[i] * widths[i] * 3);
            im.src = dev + P.frame[i];
        }
    }
    bstart[N] = (unsigned)b0; cstart[N] = (unsigned)c0;
    jpeg_enc_quant_tables(quality, reinterpret_cast<uint16_t(*)[64]>(host + P.qt));
    jpeg_enc_huffman(reinterpret_cast<JpegEncHuff*>(host + P.huff));
}

}  // namespace lwp
