"""The device entropy decoder of the JPEG reader (csrc/jpeg_entropy_kernels.hip) restated in Python, the host
pre-pass in front of it restated too, and a small baseline ENCODER that builds the synthetic streams of the tests from
coefficients in the project's layout.  The restatement follows the kernels step by step (subsequences, the sync inside a
workgroup and across workgroups with their round caps, the scan of the block starts, the write pass, the DC scan, the status)
and asserts the bounds of every read and store.  Mutation knobs build deliberately wrong decoders."""
import numpy as np

import jpeg_cases as jc

GROUP = 256                      # subsequences a workgroup takes
DEFAULT_SUBSEQ = 128
DEAD = (0xFFFFFFFF, 0, 0)        # the state behind a decoding error
ZZ = jc.ZIGZAG.tolist()


# ---------------------------------------------------------------------------------------------- reading a file's own tables
def raw_tables(data):
    """{(class, id): (counts[16], vals)} of the DHT segments in front of the scan, and the offset of the scan's first byte."""
    data = bytes(data)
    pos, out = 2, {}
    while True:
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        L = int.from_bytes(data[pos:pos + 2], "big")
        seg = data[pos + 2:pos + L]
        pos += L
        if m == 0xC4:
            while seg:
                counts = list(seg[1:17])
                n = sum(counts)
                out[(seg[0] >> 4, seg[0] & 15)] = (counts, list(seg[17:17 + n]))
                seg = seg[17 + n:]
        elif m == 0xDA:
            return out, pos


def scan_bytes(data):
    """The entropy-coded bytes of a valid file as they stand in it (stuffed, with its RSTn markers), up to EOI."""
    data = bytes(data)
    _, pos = raw_tables(data)
    assert data[-2:] == b"\xff\xd9"
    return data[pos:-2]


# ---------------------------------------------------------------------------------------------- the encoder
def _codes(counts, vals):
    """symbol -> (code, length) of a canonical table."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


SAMPLING = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}


def geometry(width, height, sampling):
    """What the header of such a file gives: components, luma sampling, MCU grid, block grids and total_blocks."""
    h0, v0 = SAMPLING[sampling]
    nc = 1 if sampling == "grey" else 3
    mx, my = -(-width // (8 * h0)), -(-height // (8 * v0))
    hs, vs = [h0, 1, 1][:nc], [v0, 1, 1][:nc]
    bw, bh = [mx * h for h in hs], [my * v for v in vs]
    return {"components": nc, "h_samp": hs, "v_samp": vs, "mcus_x": mx, "mcus_y": my, "blocks_w": bw, "blocks_h": bh,
            "total_blocks": sum(w * h for w, h in zip(bw, bh))}


def stream_order(g):
    """Plane-order block index of every block in stream (MCU) order, and its component."""
    order, comp, base = [], [], 0
    bases = []
    for c in range(g["components"]):
        bases.append(base)
        base += g["blocks_w"][c] * g["blocks_h"][c]
    for mcu in range(g["mcus_x"] * g["mcus_y"]):
        my, mx = divmod(mcu, g["mcus_x"])
        for c in range(g["components"]):
            for v in range(g["v_samp"][c]):
                for u in range(g["h_samp"][c]):
                    order.append(bases[c] + (my * g["v_samp"][c] + v) * g["blocks_w"][c] + mx * g["h_samp"][c] + u)
                    comp.append(c)
    return order, comp


SCAN_MUTANTS = ("dc11_as_dc10", "ac_code", "no_align", "final_ff_unstuffed", "zrl_at_15")


def encode_scan(coef, g, tables, td, ta, restart_interval=0, mutant=None, mutant_arg=None):
    """The scan of coefficients in the project's layout (int (total_blocks, 64), natural order, plane order, DC prediction
    undone): stuffed bytes with RSTn markers, each interval padded with one-bits.

    ``mutant`` builds a deliberately wrong coder (test_jpeg_encode_host.py shows that its named case sees each): DC category 11
    coded as category 10; the last bit of AC symbol ``mutant_arg``'s code flipped; the interval that starts at stream index
    ``mutant_arg`` not byte-aligned (the bits left over go on behind the marker); a final 0xFF without its stuffing zero; ZRL
    for a run of 15 already."""
    assert mutant is None or mutant in SCAN_MUTANTS, mutant
    coef = np.asarray(coef).astype(np.int64).tolist()
    order, comp = stream_order(g)
    per_mcu = len(order) // (g["mcus_x"] * g["mcus_y"])
    dc = [_codes(*tables[(0, td[c])]) for c in range(g["components"])]
    ac = [_codes(*tables[(1, ta[c])]) for c in range(g["components"])]
    if mutant == "dc11_as_dc10":
        for d in dc:
            d[11] = d[10]
    if mutant == "ac_code":
        for a in ac:
            a[mutant_arg] = (a[mutant_arg][0] ^ 1, a[mutant_arg][1])
    longest_run = 14 if mutant == "zrl_at_15" else 15
    out = bytearray()
    acc, nbits = 0, 0
    pred = [0] * g["components"]
    rst = 0

    def flush():
        nonlocal acc, nbits
        if nbits % 8:
            pad = 8 - nbits % 8
            acc = (acc << pad) | ((1 << pad) - 1)
            nbits += pad
        for b in acc.to_bytes(nbits // 8, "big"):
            out.append(b)
            if b == 0xFF:
                out.append(0)
        acc, nbits = 0, 0

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length

    def magnitude(v):
        s = abs(v).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    for n, (blk, c) in enumerate(zip(order, comp)):
        if restart_interval and n and n % (per_mcu * restart_interval) == 0:
            keep = nbits % 8 if mutant == "no_align" and n == mutant_arg else 0
            left = acc & ((1 << keep) - 1)
            acc, nbits = acc >> keep, nbits - keep
            flush()
            acc, nbits = left, keep
            out += bytes([0xFF, 0xD0 + rst])
            rst = (rst + 1) & 7
            pred = [0] * g["components"]
        b = coef[blk]
        s, bits = magnitude(b[0] - pred[c])
        pred[c] = b[0]
        put(*dc[c][s])
        put(bits, s)
        run = 0
        last = max([k for k in range(1, 64) if b[ZZ[k]]], default=0)
        for k in range(1, last + 1):
            v = b[ZZ[k]]
            if v == 0:
                run += 1
                continue
            while run > longest_run:
                put(*ac[c][0xF0])
                run = max(run - 16, 0)
            s, bits = magnitude(v)
            put(*ac[c][(run << 4) | s])
            put(bits, s)
            run = 0
        if last < 63:
            put(*ac[c][0x00])
    flush()
    if mutant == "final_ff_unstuffed" and out[-2:] == b"\xff\x00":
        del out[-1]
    return bytes(out)


def encode(coef, width, height, sampling, tables, qt=None, td=None, ta=None, quant_table=None, restart_interval=0):
    """A whole baseline file around encode_scan.  tables: {(class, id): (counts, vals)}; td / ta / quant_table per component
    (default: component 0 uses tables 0, the others tables 1 where defined)."""
    g = geometry(width, height, sampling)
    nc = g["components"]
    if qt is None:
        qt = np.ones((4, 64), dtype=np.uint16)
    second = 1 if (0, 1) in tables and (1, 1) in tables else 0
    td = td or [0, second, second][:nc]
    ta = ta or [0, second, second][:nc]
    quant_table = quant_table or [0, 1, 1][:nc]

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for t in sorted(set(quant_table)):
        out += seg(0xDB, [t] + [int(qt[t][ZZ[i]]) for i in range(64)])
    sof = [8] + list(height.to_bytes(2, "big")) + list(width.to_bytes(2, "big")) + [nc]
    for c in range(nc):
        sof += [c + 1, (g["h_samp"][c] << 4) | g["v_samp"][c], quant_table[c]]
    out += seg(0xC0, sof)
    for (tc, th), (counts, vals) in sorted(tables.items()):
        out += seg(0xC4, [(tc << 4) | th] + list(counts) + list(vals))
    if restart_interval:
        out += seg(0xDD, restart_interval.to_bytes(2, "big"))
    sos = [nc]
    for c in range(nc):
        sos += [c + 1, (td[c] << 4) | ta[c]]
    out += seg(0xDA, sos + [0, 63, 0])
    return out + encode_scan(coef, g, tables, td, ta, restart_interval) + b"\xff\xd9"


def standard_tables():
    """The tables libjpeg writes when it does not optimise them (ITU T.81 Annex K), read from a fixture that carries them."""
    t, _ = raw_tables(jc.fixtures()["17x17_420"][0])
    assert t[(0, 0)] == ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
    return t


def long_code_tables():
    """Tables whose rarest symbols have 16-bit codes (the canonical walk behind the 9-bit look-up): DC category 0 and the AC
    symbols with the longest runs."""
    ac_syms = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    ac_counts = [0, 1, 1, 1, 1, 1, 1, 1, 100, 0, 0, 0, 0, 0, 0, len(ac_syms) - 107]
    dc_counts = [1] * 11 + [0] * 4 + [1]
    return {(0, 0): (dc_counts, list(range(1, 12)) + [0]), (1, 0): (ac_counts, ac_syms)}


def tiny_tables():
    """A one-bit code for DC category 0 and a two-bit code for end-of-block: an all-zero block takes three bits, so block starts
    fall on every bit offset of a byte."""
    return {(0, 0): ([2] + [0] * 15, [0, 1]), (1, 0): ([0, 2] + [0] * 14, [0x00, 0x01])}


def random_coefficients(seed, g, density=1.0, sizes=(1, 10), dc=1000, all_ones=False):
    rng = np.random.RandomState(seed)
    n = g["total_blocks"]
    s = rng.randint(sizes[0], sizes[1] + 1, size=(n, 64))
    mag = (1 << s) - 1 if all_ones else rng.randint(0, 1 << 30, size=(n, 64)) % (1 << (s - 1)) + (1 << (s - 1))
    sign = np.ones((n, 64), dtype=np.int64) if all_ones else rng.choice([-1, 1], size=(n, 64))
    coef = (mag * sign * (rng.rand(n, 64) < density)).astype(np.int64)
    coef[:, 0] = rng.randint(-dc, dc + 1, size=n)
    return coef.astype(np.int16)


_PARSED = {}


def parse(data):
    """jpeg_cases.parse, computed once per header: the bit-flip mutants of a file share theirs."""
    _, pos = raw_tables(data)
    key = bytes(data[:pos])
    if key not in _PARSED:
        _PARSED[key] = jc.parse(data)
    return _PARSED[key]


# ---------------------------------------------------------------------------------------------- the pre-pass restated
def scan_segments(data):
    """jpeg_scan_segments: (status, un-stuffed bytes, [(byte offset, byte length, first MCU, MCU count)]); bytes and segments
    are unspecified for a refused file."""
    data = bytes(data)
    hd, _, _, pos = parse(data)
    n = len(data)
    n_mcus = hd["mcus_x"] * hd["mcus_y"]
    ri = hd["restart_interval"]
    expected = -(-n_mcus // ri) if ri else 1
    if hd["total_blocks"] > 4 * (n - pos):
        return 1, b"", []
    out, segs, seg_out, next_rst = bytearray(), [], 0, 0

    def close():
        nonlocal seg_out
        first = len(segs) * ri
        segs.append((seg_out, len(out) - seg_out, first, min(ri, n_mcus - first) if ri else n_mcus))
        seg_out = len(out)
    while True:
        stop = data.find(b"\xff", pos)
        stop = n if stop < 0 else stop
        out += data[pos:stop]
        pos = stop
        if pos + 1 >= n:
            return 1, bytes(out), segs
        if data[pos + 1] == 0:
            out.append(0xFF)
            pos += 2
            continue
        q = pos
        while q < n and data[q] == 0xFF:
            q += 1
        if q >= n:
            return 1, bytes(out), segs
        m = data[q]
        if 0xD0 <= m <= 0xD7:
            if not ri or len(segs) + 1 >= expected or m != 0xD0 + next_rst:
                return 1, bytes(out), segs
            close()
            next_rst = (next_rst + 1) & 7
            pos = q + 1
            continue
        close()
        if len(segs) != expected:
            return 1, bytes(out), segs
        break
    while True:                                           # the trailer up to EOI
        if pos >= n or data[pos] != 0xFF:
            return 1, bytes(out), segs
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return 1, bytes(out), segs
        m = data[pos]
        pos += 1
        if m == 0xD9:
            return 0, bytes(out), segs
        if m in (0xDA, 0xDC, 0x00, 0x01, 0xD8) or 0xD0 <= m <= 0xD7:
            return 1, bytes(out), segs
        if n - pos < 2:
            return 1, bytes(out), segs
        L = int.from_bytes(data[pos:pos + 2], "big")
        if L < 2 or L > n - pos:
            return 1, bytes(out), segs
        pos += L


def flat_table(counts, vals):
    """JpegHuffFlat of one table as 1488 bytes."""
    look = np.zeros(512, dtype=np.uint16)
    maxcode, mincode, valptr = np.full(17, 0, np.int32), np.zeros(17, np.int32), np.zeros(17, np.int32)
    maxcode[0] = -1
    code, k = 0, 0
    for l in range(1, 17):
        valptr[l], mincode[l] = k, code
        if counts[l - 1]:
            if l <= 9:
                for i in range(counts[l - 1]):
                    first = (code + i) << (9 - l)
                    look[first:first + (1 << (9 - l))] = (l << 8) | vals[k + i]
            code += counts[l - 1]
            maxcode[l] = code - 1
            k += counts[l - 1]
        else:
            maxcode[l] = -1
        code <<= 1
    v = np.zeros(256, dtype=np.uint8)
    v[:len(vals)] = vals
    return look.tobytes() + maxcode.tobytes() + mincode.tobytes() + valptr.tobytes() + v.tobytes() + bytes(4)


# ---------------------------------------------------------------------------------------------- the kernels restated
class Decoder:
    """One file through the four kernels.  ``subseq``: bytes a lane owns; ``group``: lanes a workgroup."""

    def __init__(self, data, subseq=DEFAULT_SUBSEQ, group=GROUP, ignore_k=False, ignore_block=False, no_stitch=False,
                 dc_plane_order=False):
        assert 4 <= subseq <= 1024 and subseq % 4 == 0
        self.data = bytes(data)
        self.S, self.G = subseq, group
        self.ignore_k, self.ignore_block, self.no_stitch, self.dc_plane_order = ignore_k, ignore_block, no_stitch, dc_plane_order
        self.hd, self.qt, self.huff, _ = parse(self.data)
        hd = self.hd
        self.nc = hd["components"]
        self.luma = hd["h_samp"][0] * hd["v_samp"][0] if self.nc > 1 else 1
        self.bpm = self.luma + 2 if self.nc > 1 else 1
        self.total = hd["total_blocks"]
        self.plane0 = [0]
        for c in range(self.nc - 1):
            self.plane0.append(self.plane0[-1] + hd["blocks_w"][c] * hd["blocks_h"][c])
        self.rounds = [0, 0]

    def same(self, a, b):
        if self.ignore_k:
            return a[:2] == b[:2]
        if self.ignore_block:
            return (a[0], a[2]) == (b[0], b[2])
        return a == b

    def component(self, bim):
        return 0 if self.nc == 1 or bim < self.luma else min(1 + bim - self.luma, 2)

    def address(self, n):
        """ent_block_address: the plane-order address of the block with stream index n, total_blocks: none."""
        hd = self.hd
        mcu, b = divmod(n, self.bpm)
        my, mx = divmod(mcu, hd["mcus_x"])
        c, u, v, hs, vs = 0, 0, 0, 1, 1
        if self.nc > 1:
            if b < self.luma:
                v, u = divmod(b, hd["h_samp"][0])
                hs, vs = hd["h_samp"][0], hd["v_samp"][0]
            else:
                c = min(1 + b - self.luma, 2)
        a = self.plane0[c] + (my * vs + v) * hd["blocks_w"][c] + mx * hs + u
        return a if a < self.total else self.total

    def peek(self, seg, pos):
        """32 bits at bit position pos of the segment's bytes, zero past its end."""
        seg_bits = 8 * len(seg)
        if pos >= seg_bits:
            return 0
        p = pos >> 3
        assert 0 <= p < len(seg)
        w = int.from_bytes(seg[p:p + 5].ljust(5, b"\0"), "big")
        return (w >> (8 - (pos & 7))) & 0xFFFFFFFF

    def decode(self, seg, st, limit, w=None):
        """ent_decode: from state st while the bit position is below limit; returns (exit state, block starts seen).  w: the
        write pass's side, a dict of n, end, cur, bad, finished."""
        seg_bits = 8 * len(seg)
        pos, bim, k = st
        count = 0
        turns = 0
        while pos < limit:
            turns += 1
            assert turns <= limit + 1                     # at least one bit a turn
            if w is not None:
                if w["n"] > w["end"]:
                    break
                if w["n"] == w["end"] and k == 0:
                    if seg_bits - pos >= 8:
                        w["bad"] = True
                    w["finished"] = True
                    break
            bits = self.peek(seg, pos)
            c = self.component(bim)
            length, symbol = self.huff[(0, self.hd["td"][c])] if k == 0 else self.huff[(1, self.hd["ta"][c])]
            l, sym = length[bits >> 16], symbol[bits >> 16]
            err = l == 0
            sz = 0
            if not err:
                if k == 0:
                    sz = sym
                    err = sz > 11
                else:
                    r, sz = sym >> 4, sym & 15
                    if sz == 0:
                        if r == 15:
                            k += 16
                            err = k > 63
                        else:
                            k = 64
                    else:
                        k += r
                        err = k > 63 or sz > 10
            if not err:
                err = pos + l + sz > seg_bits
            if err:
                if w is not None:
                    w["bad"] = True
                pos, bim, k = DEAD
                break
            val = 0
            if sz:
                raw = ((bits << l) & 0xFFFFFFFF) >> (32 - sz)
                val = raw - (1 << sz) + 1 if raw < (1 << (sz - 1)) else raw
            pos += l + sz
            if k == 0:
                count += 1
                if w is not None:
                    w["cur"] = self.address(w["n"])
                    w["n"] += 1
                    if w["cur"] < self.total:
                        self.store(w["cur"], 0, val)
                k = 1
            elif sz:
                if w is not None and w["cur"] < self.total and k <= 63:
                    self.store(w["cur"], ZZ[k], val)
                k += 1
            if k >= 64:
                k, bim = 0, (0 if bim + 1 == self.bpm else bim + 1)
        return (pos, bim, k), count

    def store(self, block, at, val):
        assert 0 <= block < self.total and 0 <= at < 64
        self.coef[block, at] = val

    def run(self):
        """(status, coefficients): status 0 accepted; the coefficients as the library lays them out."""
        status, raw, scan = scan_segments(self.data)
        if status:
            return status, None
        S8 = self.S * 8
        segs = []                                          # (bytes, first block, blocks, first subsequence)
        n_subs = 0
        for byte0, n_bytes, first_mcu, n_mcus in scan:
            segs.append((raw[byte0:byte0 + n_bytes], first_mcu * self.bpm, n_mcus * self.bpm, n_subs))
            n_subs += max(1, -(-n_bytes // self.S))
        seg_of, first_of, last_of, limits, starts = [], [], [], [], []
        for si, (b, _, _, sub0) in enumerate(segs):
            cnt = max(1, -(-len(b) // self.S))
            for j in range(cnt):
                seg_of.append(si)
                first_of.append(j == 0)
                last_of.append(j == cnt - 1)
                starts.append(j * S8)
                limits.append(8 * len(b) if j == cnt - 1 else min((j + 1) * S8, 8 * len(b)))
        rec = [None] * n_subs                              # (exit, count)
        n_wgs = -(-n_subs // self.G)
        # 1. sync inside a workgroup
        for wg in range(n_wgs):
            lanes = range(wg * self.G, min((wg + 1) * self.G, n_subs))
            used = {g: (starts[g], 0, 0) for g in lanes}
            for g in lanes:
                rec[g] = self.decode(segs[seg_of[g]][0], used[g], limits[g])
            rounds = 1
            while rounds <= self.G:
                entries = {g: rec[g - 1][0] for g in lanes if not first_of[g] and g != lanes[0]}
                changed = False
                for g, entry in entries.items():
                    if not self.same(entry, used[g]):
                        used[g] = entry
                        rec[g] = self.decode(segs[seg_of[g]][0], entry, limits[g])
                        changed = True
                if not changed:
                    break
                rounds += 1
            self.rounds[0] = max(self.rounds[0], rounds)
        # 2. sync across workgroups
        if not self.no_stitch:
            wg_entry = {}
            rounds = 0
            for _ in range(n_wgs - 1):
                dirty = []
                for wg in range(1, n_wgs):
                    g = wg * self.G
                    if not first_of[g] and rec[g - 1][0] != wg_entry.get(wg):
                        wg_entry[wg] = rec[g - 1][0]
                        dirty.append(wg)
                rounds += 1
                if not dirty:
                    break
                for wg in dirty:
                    st = wg_entry[wg]
                    g = wg * self.G
                    while g < min((wg + 1) * self.G, n_subs) and seg_of[g] == seg_of[wg * self.G]:
                        new = self.decode(segs[seg_of[g]][0], st, limits[g])
                        old, rec[g] = rec[g], new
                        if self.same(new[0], old[0]):
                            break
                        st = new[0]
                        g += 1
            self.rounds[1] = rounds
        # positions: an exclusive scan over the file's subsequences
        subpos, acc = [], 0
        for g in range(n_subs):
            subpos.append(acc)
            acc += rec[g][1]
        # 3. the write pass
        self.coef = np.zeros((self.total, 64), dtype=np.int64)
        bad = False
        for g in range(n_subs):
            b, first_block, n_blocks, sub0 = segs[seg_of[g]]
            st = (0, 0, 0) if first_of[g] else rec[g - 1][0]
            w = {"n": first_block + subpos[g] - subpos[sub0], "end": first_block + n_blocks, "cur": self.total, "bad": False,
                 "finished": False}
            if st[2] != 0 and 1 <= w["n"] <= w["end"]:
                w["cur"] = self.address(w["n"] - 1)
            if st == DEAD and last_of[g]:
                w["bad"] = True
            st, _ = self.decode(b, st, limits[g], w)
            if last_of[g] and not w["finished"] and w["n"] <= w["end"] and not (w["n"] == w["end"] and st[2] == 0 and st[0] != DEAD[0]):
                w["bad"] = True
            bad = bad or w["bad"]
        # 4. the DC scan: per segment and component, in stream order
        hd = self.hd
        for b, first_block, n_blocks, sub0 in segs:
            mcu0, n_mcus = first_block // self.bpm, n_blocks // self.bpm
            in_mcu0 = 0
            for c in range(self.nc):
                hv = self.luma if c == 0 and self.nc > 1 else 1
                addrs = [self.address((mcu0 + i // hv) * self.bpm + in_mcu0 + i % hv) for i in range(n_mcus * hv)]
                if self.dc_plane_order:
                    addrs = sorted(addrs)
                run = 0
                for a in addrs:
                    assert 0 <= a < self.total
                    run = ((run + int(self.coef[a, 0]) + (1 << 31)) % (1 << 32)) - (1 << 31)
                    if run < -2048 or run > 2047:
                        bad = True
                    self.coef[a, 0] = ((run + (1 << 15)) % (1 << 16)) - (1 << 15)
                in_mcu0 += hv
        if bad:
            return 1, None
        return 0, self.coef.astype(np.int16)


def device_decode(data, subseq=DEFAULT_SUBSEQ, **knobs):
    return Decoder(data, subseq, **knobs).run()


def bit_flips(data):
    """Every single-bit flip of the scan bytes of a valid file (the trailing EOI excluded)."""
    data = bytes(data)
    _, start = raw_tables(data)
    for at in range(start, len(data) - 2):
        for bit in range(8):
            yield data[:at] + bytes([data[at] ^ (1 << bit)]) + data[at + 1:]


# ---------------------------------------------------------------------------------------------- synthetic streams
_SYNTHETIC = None


def synthetic():
    """{name: file bytes} of the streams the fixtures do not have, built once per process by the encoder."""
    global _SYNTHETIC
    if _SYNTHETIC is not None:
        return _SYNTHETIC
    std = standard_tables()
    out = {}

    def add(name, seed, w, h, sampling, tables=std, ri=0, **how):
        g = geometry(w, h, sampling)
        out[name] = encode(random_coefficients(seed, g, **how), w, h, sampling, tables, restart_interval=ri)
    # all 63 AC coefficients at size 10: a block spans many subsequences, and some subsequences see no block start
    add("size10_420", 1, 64, 48, "420", sizes=(10, 10))
    add("size10_grey", 2, 40, 24, "grey", sizes=(10, 10))
    add("size10_444", 3, 40, 24, "444", sizes=(10, 10))
    add("size10_422", 4, 40, 24, "422", sizes=(10, 10))
    # end-of-block only, three bits a block (six with the standard tables): hundreds of block starts a subsequence
    g = geometry(512, 512, "grey")
    out["eob_only_grey"] = encode(np.zeros((g["total_blocks"], 64), dtype=np.int16), 512, 512, "grey", tiny_tables())
    g = geometry(64, 64, "420")
    out["eob_only_420"] = encode(np.zeros((g["total_blocks"], 64), dtype=np.int16), 64, 64, "420", std)
    # a chroma block that starts on the first bit of a 4-byte subsequence: only the block index tells its state from the cold one
    add("block_sync_444", 135, 32, 32, "444", density=0.5)
    # magnitude bits all ones: a scan dense in stuffed FF 00
    add("all_ones_444", 5, 32, 32, "444", all_ones=True, density=0.6)
    # 16-bit codes: the canonical walk behind the look-up
    add("long_codes_grey", 6, 48, 48, "grey", tables=long_code_tables(), density=0.3)
    # every segment a single subsequence; segments longer than a workgroup's 256 subsequences (at 4 bytes a subsequence)
    add("restart1_420", 7, 48, 32, "420", ri=1, density=0.2, sizes=(1, 6))
    add("restart64_grey", 8, 128, 128, "grey", ri=64, density=0.8)
    # several workgroup boundaries at the default subsequence: a scan of more than 3 * 256 * 128 bytes
    add("big_420", 9, 256, 256, "420")
    _SYNTHETIC = out
    return out
