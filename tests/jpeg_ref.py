"""numpy restatement of the baseline JPEG front end of include/mec.h: mec_jpeg_probe (which files the GPU decodes,
their descriptors and restart segments) and mec_jpeg_decode_ragged (entropy decoding, libjpeg's slow-integer IDCT,
fancy upsampling and YCbCr -> RGB, all integer arithmetic, and the status conditions). Written from the header's
statement and the JPEG standard, independent of csrc/jpeg.hip; the tests hold it against Pillow's pixels and the
kernels against it."""
import numpy as np

# zigzag position -> natural (row-major) index of an 8 x 8 block
NATURAL = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8 if (i // 8 + i % 8) % 2 else i % 8))), np.int32)

# status codes (include/mec.h MEC_JPEG_ST_*)
OK, BAD_CODE, DC_CATEGORY, AC_SIZE, COEF_INDEX, SEGMENT_END, IDCT_RANGE, COEF_RANGE = range(8)


class Desc:
    """One file's descriptor: H, W, ncomp, hs[c], vs[c], qt[c] (64 values in zigzag order), dc[c] / ac[c]
    ((16 counts, values)), restart (MCUs, 0: none), segs [(offset, length)] into the file's bytes."""

    def __init__(self):
        self.H = self.W = self.ncomp = self.restart = 0
        self.hs, self.vs, self.qt, self.dc, self.ac, self.segs = [], [], [], [], [], []

    def mcus(self):
        hmax, vmax = max(self.hs), max(self.vs)
        return -(-self.W // (8 * hmax)), -(-self.H // (8 * vmax))


def resize_on_gpu(H, W):
    return 1 <= H <= 4096 and 1 <= W <= 4096 and H <= 100 * W


def _huff_ok(counts):
    code = 0
    last = max([l for l in range(16) if counts[l]], default=-1)
    for l in range(last + 1):
        code += counts[l]
        if code >= 1 << (l + 1):
            return False
        code <<= 1
    return True


def probe(data):
    """bytes -> Desc, or None for a file that goes to the host."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return None
    pos = 2
    qts, huff = {}, {}
    frame = None
    restart = 0
    while True:
        if pos >= n or d[pos] != 0xFF:
            return None
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return None
        m = d[pos]
        pos += 1
        if not (m in (0xC0, 0xC4, 0xDB, 0xDD, 0xDA, 0xFE) or (0xE0 <= m <= 0xEF and m != 0xEE)):
            return None
        if pos + 2 > n:
            return None
        L = (d[pos] << 8) | d[pos + 1]
        if L < 2 or pos + L > n:
            return None
        seg = d[pos + 2:pos + L]
        pos += L
        if m == 0xC0:
            if frame is not None or len(seg) < 6:
                return None
            P, H, W, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if P != 8 or nf not in (1, 3) or len(seg) != 6 + 3 * nf:
                return None
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)]
            if any(tq > 3 for _, _, _, tq in comps):
                return None
            if nf == 1:
                if comps[0][1:3] != (1, 1):
                    return None
            else:
                if [c[0] for c in comps] != [1, 2, 3] or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
                    return None
                if comps[0][1:3] not in ((1, 1), (2, 1), (2, 2)):
                    return None
            if not resize_on_gpu(H, W) or (comps[0][1] == 2 and W < 5):
                return None
            frame = (H, W, comps)
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    return None
                tc, th = seg[at] >> 4, seg[at] & 15
                counts = list(seg[at + 1:at + 17])
                nv = sum(counts)
                if tc > 1 or th > 1 or nv > 256 or at + 17 + nv > len(seg) or not _huff_ok(counts):
                    return None
                huff[(tc, th)] = (counts, list(seg[at + 17:at + 17 + nv]))
                at += 17 + nv
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                if seg[at] >> 4 != 0 or (seg[at] & 15) > 3 or at + 65 > len(seg):
                    return None
                qts[seg[at] & 15] = list(seg[at + 1:at + 65])
                at += 65
        elif m == 0xDD:
            if len(seg) != 2:
                return None
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if frame is None:
                return None
            H, W, comps = frame
            nf = len(comps)
            if len(seg) != 4 + 2 * nf or seg[0] != nf:
                return None
            out = Desc()
            out.H, out.W, out.ncomp, out.restart = H, W, nf, restart
            for i, (cid, h, v, tq) in enumerate(comps):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if seg[1 + 2 * i] != cid or td > 1 or ta > 1:
                    return None
                if tq not in qts or (0, td) not in huff or (1, ta) not in huff:
                    return None
                out.hs.append(h)
                out.vs.append(v)
                out.qt.append(qts[tq])
                out.dc.append(huff[(0, td)])
                out.ac.append(huff[(1, ta)])
            if seg[1 + 2 * nf] != 0 or seg[2 + 2 * nf] != 63 or seg[3 + 2 * nf] != 0:
                return None
            break
    # the entropy-coded data, up to the next marker that is no RSTn
    start, expect, p = pos, 0, pos
    while True:
        if p >= n:
            return None
        if d[p] != 0xFF:
            p += 1
            continue
        q = p
        while q < n and d[q] == 0xFF:
            q += 1
        if q >= n:
            return None
        b = d[q]
        if b == 0:
            if q != p + 1:
                return None  # fill bytes before a stuffed zero
            p = q + 1
            continue
        out.segs.append((start, p - start))
        if 0xD0 <= b <= 0xD7:
            if restart == 0 or b != 0xD0 + expect:
                return None
            expect = (expect + 1) & 7
            start = p = q + 1
            continue
        if b != 0xD9:
            return None
        break
    mx, my = out.mcus()
    if len(out.segs) != (-(-(mx * my) // restart) if restart else 1):
        return None
    return out


class _Table:
    def __init__(self, counts, vals):
        self.maxcode, self.valptr, self.mincode, self.vals = [], [], [], vals
        code = p = 0
        for l in range(16):
            self.valptr.append(p)
            self.mincode.append(code)
            p += counts[l]
            code += counts[l]
            self.maxcode.append(code - 1 if counts[l] else -1)
            code <<= 1


class _Bits:
    """MSB-first bit reader over one segment; a byte after 0xFF is dropped (the stuffed zero)."""

    def __init__(self, d, off, n):
        raw = d[off:off + n]
        b, i = bytearray(), 0
        while i < len(raw):
            if raw[i] == 0xFF:
                if i + 1 >= len(raw):
                    break  # an 0xFF without its stuffed byte: the segment ends here
                b.append(0xFF)
                i += 2
            else:
                b.append(raw[i])
                i += 1
        self.b, self.pos, self.nbits = bytes(b), 0, 8 * len(b)

    def take(self, k):
        if self.pos + k > self.nbits:
            return None
        v = 0
        for _ in range(k):
            v = (v << 1) | ((self.b[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def symbol(self, t):
        code = 0
        for l in range(16):
            bit = self.take(1)
            if bit is None:
                return None, SEGMENT_END
            code = (code << 1) | bit
            if t.maxcode[l] >= 0 and t.mincode[l] <= code <= t.maxcode[l]:
                return t.vals[t.valptr[l] + code - t.mincode[l]], OK
        return None, BAD_CODE


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy(desc, data):
    """-> (status, [per component int32 coefficients [bh, bw, 64], natural order, not dequantized])."""
    d = bytes(data)
    mx, my = desc.mcus()
    if desc.ncomp == 1:
        dims = [(-(-desc.H // 8), -(-desc.W // 8))]
        mx, my = dims[0][1], dims[0][0]
        order = [(0, 0, 0)]
    else:
        dims = [(my * desc.vs[c], mx * desc.hs[c]) for c in range(3)]
        order = [(c, v, h) for c in range(3) for v in range(desc.vs[c]) for h in range(desc.hs[c])]
    coef = [np.zeros((bh, bw, 64), np.int32) for bh, bw in dims]
    dct = [_Table(*t) for t in desc.dc]
    act = [_Table(*t) for t in desc.ac]
    per = desc.restart if desc.restart else mx * my
    for si, (off, n) in enumerate(desc.segs):
        br = _Bits(d, off, n)
        pred = [0] * desc.ncomp
        for mcu in range(si * per, min((si + 1) * per, mx * my)):
            yy, xx = divmod(mcu, mx)
            for c, v, h in order:
                blk = coef[c][yy * (desc.vs[c] if desc.ncomp == 3 else 1) + v, xx * (desc.hs[c] if desc.ncomp == 3 else 1) + h]
                s, st = br.symbol(dct[c])
                if st:
                    return st, None
                if s > 11:
                    return DC_CATEGORY, None
                if s:
                    v_ = br.take(s)
                    if v_ is None:
                        return SEGMENT_END, None
                    pred[c] += _extend(v_, s)
                if not -32768 <= pred[c] <= 32767:
                    return COEF_RANGE, None
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs, st = br.symbol(act[c])
                    if st:
                        return st, None
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    if s > 10:
                        return AC_SIZE, None
                    k += r
                    if k > 63:
                        return COEF_INDEX, None
                    v_ = br.take(s)
                    if v_ is None:
                        return SEGMENT_END, None
                    blk[NATURAL[k]] = _extend(v_, s)
                    k += 1
    return OK, coef


def _fix(x):
    return int(x * 8192 + 0.5)


F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175, F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = map(_fix, (
    0.298631336, 0.390180644, 0.541196100, 0.765366865, 0.899976223, 1.175875602, 1.501321110, 1.847759065,
    1.961570560, 2.053119869, 2.562915447, 3.072711026))


def _pass(x, shift):
    """jidctint's 1-D pass over the last axis of int64 x [..., 8]; descale by `shift`."""
    x = [x[..., i] for i in range(8)]
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * F_0_541
    tmp2 = z1 - z3 * F_1_847
    tmp3 = z1 + z2 * F_0_765
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298, tmp1 * F_2_053, tmp2 * F_3_072, tmp3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + (1 << (shift - 1))) >> shift for o in out], -1)


def idct(coef, qt):
    """int coefficients [bh, bw, 64] (natural order), qt 64 values in zigzag order -> (status, u8 plane
    [bh * 8, bw * 8])."""
    q = np.zeros(64, np.int64)
    q[NATURAL] = np.asarray(qt, np.int64)
    x = coef.astype(np.int64) * q
    if (x < -32768).any() or (x > 32767).any():
        return COEF_RANGE, None
    bh, bw = x.shape[:2]
    x = x.reshape(bh, bw, 8, 8)
    ws = _pass(x.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)  # columns
    if (ws < -32768).any() or (ws > 32767).any():
        return IDCT_RANGE, None
    o = _pass(ws, 18)  # rows
    if (o < -512).any() or (o > 511).any():
        return IDCT_RANGE, None
    o = np.clip(o + 128, 0, 255).astype(np.uint8)
    return OK, o.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1(p):
    """fancy h2v1 of an int plane [dh, dw] -> [dh, 2 dw]."""
    c = p.astype(np.int64)
    prev = np.concatenate([c[:, :1], c[:, :-1]], 1)
    nxt = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + prev + 1) >> 2
    out[:, 1::2] = (3 * c + nxt + 2) >> 2
    out[:, 0] = c[:, 0]
    out[:, -1] = c[:, -1]
    return out


def _h2v2(p):
    """fancy h2v2 of an int plane [dh, dw] -> [2 dh, 2 dw]."""
    c = p.astype(np.int64)
    up = np.concatenate([c[:1], c[:-1]], 0)
    dn = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    for par, far in ((0, up), (1, dn)):
        s = 3 * c + far
        prev = np.concatenate([s[:, :1], s[:, :-1]], 1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + prev + 8) >> 4, (3 * s + nxt + 7) >> 4
        even[:, 0] = (4 * s[:, 0] + 8) >> 4
        odd[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[par::2, 0::2] = even
        out[par::2, 1::2] = odd
    return out


def _f16(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_f16(1.402) * cr + 32768) >> 16)
    b = y + ((_f16(1.772) * cb + 32768) >> 16)
    g = y + ((-_f16(0.34414) * cb - _f16(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(desc, data):
    """-> (status, u8 [H, W, C] or None where status is nonzero)."""
    st, coef = entropy(desc, data)
    if st:
        return st, None
    planes = []
    for c in range(desc.ncomp):
        st, p = idct(coef[c], desc.qt[c])
        if st:
            return st, None
        planes.append(p)
    H, W = desc.H, desc.W
    if desc.ncomp == 1:
        return OK, planes[0][:H, :W, None].copy()
    hmax, vmax = desc.hs[0], desc.vs[0]
    dw, dh = -(-W // hmax), -(-H // vmax)
    ch = []
    for p in planes[1:]:
        p = p[:dh, :dw]
        if (hmax, vmax) == (2, 1):
            p = _h2v1(p)
        elif (hmax, vmax) == (2, 2):
            p = _h2v2(p)
        ch.append(p[:H, :W])
    return OK, colour(planes[0][:H, :W], ch[0], ch[1])


def decode_file(data):
    """bytes -> (Desc or None, status, pixels)."""
    desc = probe(data)
    if desc is None:
        return None, None, None
    st, px = decode(desc, data)
    return desc, st, px
