"""The entropy-coded wire format (include/bvcodec.h, "Entropy-coded wire format") in numpy and plain integers: test infrastructure.
The encoder and the decoder are written separately from the specification; neither calls the other.  The encoder reports whether a
carry went through a run of 0xFF bytes (the path a range coder most easily gets wrong)."""
import numpy as np

TOP = 1 << 24
MASK32 = 0xFFFFFFFF


def quantise(p):
    """q = clamp(rint(p * 65536), 1, 65535) of float32 p, P(bit = 1); the product is exact in float32, rint is round-half-even."""
    x = np.rint(np.asarray(p, dtype=np.float32) * np.float32(65536.0))
    x = np.where(np.isnan(x), np.float32(1.0), x)
    return np.clip(x, 1.0, 65535.0).astype(np.int64)


def coded_mask(bits, z_dim):
    """(B, T, z_dim) bool: position n of frame t carries a bit where bits[b, t] > n.  bits None: a fixed-rate model, every position."""
    if bits is None:
        raise ValueError("pass bits (B, T); a fixed-rate model has z_dim everywhere")
    b = np.asarray(bits, dtype=np.float32)
    return b[:, :, None] > np.arange(z_dim, dtype=np.float32)[None, None, :]


def safe_stride(z_dim, segment):
    return 2 * segment * z_dim + segment // 16 + 8


def encode_segment(symbols, qs):
    """symbols, qs: sequences of 0 / 1 and of quantised probabilities.  Returns (stored bytes, carried): the emitted bytes without the
    first (always 0) and without trailing zeros; carried: a carry was added to at least one pending 0xFF."""
    low, rng, cache, cache_size = 0, MASK32, 0, 1
    out = []
    carried = False

    def shift_low():
        nonlocal low, cache, cache_size, carried
        if (low & MASK32) < 0xFF000000 or (low >> 32) != 0:
            carry = low >> 32
            out.append((cache + carry) & 0xFF)
            if cache_size > 1 and carry:
                carried = True
            out.extend([(0xFF + carry) & 0xFF] * (cache_size - 1))
            cache = (low >> 24) & 0xFF
            cache_size = 0
        cache_size += 1
        low = (low & 0x00FFFFFF) << 8

    for b, q in zip(symbols, qs):
        bound = (rng >> 16) * (65536 - int(q))
        if not b:
            rng = bound
        else:
            low += bound
            rng -= bound
        while rng < TOP:
            shift_low()
            rng = (rng << 8) & MASK32
    for _ in range(5):
        shift_low()
    assert out[0] == 0
    out = out[1:]
    while out and out[-1] == 0:
        out.pop()
    return bytes(out), carried


def decode_segment(data, qs):
    """data: the stored bytes of one segment; qs: the quantised probabilities of its coded positions, in order.  Returns the bits."""
    n = len(data)
    pos = 4
    code = 0
    for i in range(4):
        code = (code << 8) | (data[i] if i < n else 0)
    rng = MASK32
    bits = []
    for q in qs:
        bound = (rng >> 16) * (65536 - int(q))
        if code < bound:
            rng = bound
            bits.append(0)
        else:
            code -= bound
            rng -= bound
            bits.append(1)
        while rng < TOP:
            code = ((code << 8) | (data[pos] if pos < n else 0)) & MASK32
            pos += 1
            rng = (rng << 8) & MASK32
    return bits


def segments(T, segment):
    S = T if segment is None else min(int(segment), T)
    return S, [(a, min(a + S, T)) for a in range(0, T, S)]


def pack(codes, prob, bits, segment=None, stride=None):
    """codes / prob (B,T,Z) float32, bits (B,T).  Returns dict(data (B,nseg,stride) uint8, sizes (B,nseg) int32, carried (B,nseg) bool,
    ideal (B,nseg) float64 = sum of -log2 of the quantised probability of every coded bit, n (B,nseg) coded bits).  stride None: the
    safe stride; a segment that does not fit gets size -1 and only its first `stride` bytes."""
    codes, prob = np.asarray(codes, dtype=np.float32), np.asarray(prob, dtype=np.float32)
    B, T, Z = codes.shape
    S, segs = segments(T, segment)
    stride = safe_stride(Z, S) if stride is None else int(stride)
    mask = coded_mask(bits, Z)
    q = quantise(prob)
    sym = codes > np.float32(0.5)
    cost = -np.log2(np.where(sym, q, 65536 - q) / 65536.0)
    data = np.zeros((B, len(segs), stride), dtype=np.uint8)
    out = dict(data=data, sizes=np.zeros((B, len(segs)), dtype=np.int32), carried=np.zeros((B, len(segs)), dtype=bool),
               ideal=np.zeros((B, len(segs))), n=np.zeros((B, len(segs)), dtype=np.int64))
    for b in range(B):
        for s, (a, e) in enumerate(segs):
            m = mask[b, a:e].reshape(-1)
            stored, carried = encode_segment(sym[b, a:e].reshape(-1)[m].tolist(), q[b, a:e].reshape(-1)[m].tolist())
            keep = stored[:stride]
            data[b, s, :len(keep)] = np.frombuffer(keep, dtype=np.uint8)
            out["sizes"][b, s] = len(stored) if len(stored) <= stride else -1
            out["carried"][b, s] = carried
            out["ideal"][b, s] = cost[b, a:e].reshape(-1)[m].sum()
            out["n"][b, s] = int(m.sum())
    return out


def unpack(data, sizes, prob, bits, segment=None):
    """The inverse: codes (B,T,Z) float32 with 0.5 at the positions without a bit.  A size outside [0, stride] reads as 0 bytes."""
    prob = np.asarray(prob, dtype=np.float32)
    B, T, Z = prob.shape
    _, segs = segments(T, segment)
    mask = coded_mask(bits, Z)
    q = quantise(prob)
    codes = np.full((B, T, Z), 0.5, dtype=np.float32)
    for b in range(B):
        for s, (a, e) in enumerate(segs):
            m = mask[b, a:e].reshape(-1)
            n = int(sizes[b, s])
            n = n if 0 <= n <= data.shape[2] else 0
            got = decode_segment(bytes(data[b, s, :n]), q[b, a:e].reshape(-1)[m].tolist())
            frame = codes[b, a:e].reshape(-1)
            frame[m] = np.asarray(got, dtype=np.float32)
            codes[b, a:e] = frame.reshape(e - a, Z)
    return codes


# the overhead bound per segment: 8 * size <= ideal + TRUNC * n + FLUSH.  range >> 16 >= 256, so truncating range to its upper 16 bits
# loses at most log2(1 + 1/255) = 0.00565 bit per symbol; the flush costs at most 32 bits.
TRUNC, FLUSH = 0.0057, 32.0


def overhead_ok(sizes, ideal, n):
    return 8.0 * np.asarray(sizes, dtype=np.float64) <= np.asarray(ideal) + TRUNC * np.asarray(n) + FLUSH


# ---- the cases shared by the CPU and the GPU tests
PROB_CLASSES = ("flat", "skewed", "half", "extreme")
BIT_COUNTS = (0.0, 1.0, 34.5, None, 1000.0)          # None: z_dim


def prob_case(kind, B, T, Z, seed):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        p = rng.uniform(0.0, 1.0, size=(B, T, Z))
    elif kind == "skewed":
        p = rng.beta(0.08, 0.08, size=(B, T, Z))
    elif kind == "half":
        p = np.full((B, T, Z), 0.5)
    else:
        p = rng.choice(np.array([0.0, 1.0, 1e-6, 1.0 - 1e-6]), size=(B, T, Z))
    return p.astype(np.float32)


def draw_codes(p, seed, wrong=0.0):
    """Bits drawn from the quantised probabilities (a share `wrong` of them flipped: an extreme prior that is wrong costs 16 bits)."""
    rng = np.random.default_rng(seed + 1)
    sym = rng.uniform(0.0, 1.0, size=p.shape) * 65536.0 < quantise(p)
    sym ^= rng.uniform(0.0, 1.0, size=p.shape) < wrong
    return sym.astype(np.float32)


def bits_case(B, T, Z):
    """(B, T): the bit counts of BIT_COUNTS, walked so that every row and every segment sees several of them."""
    v = [float(Z) if c is None else c for c in BIT_COUNTS]
    return np.array([[v[(b + 2 * t) % len(v)] for t in range(T)] for b in range(B)], dtype=np.float32)


def masked(codes, bits):
    """codes with 0.5 at the positions without a bit: what a decoder gives back."""
    return np.where(coded_mask(bits, codes.shape[2]), codes, np.float32(0.5)).astype(np.float32)


# the carry case: 2240 symbols in one segment (35 frames of 64), uniform p, bits drawn from q
CARRY_SEED = 8


def carry_case():
    rng = np.random.default_rng(CARRY_SEED)
    p = rng.uniform(0.0, 1.0, size=(1, 35, 64)).astype(np.float32)
    sym = (rng.uniform(0.0, 1.0, size=p.shape) * 65536.0 < quantise(p)).astype(np.float32)
    return sym, p, np.full((1, 35), 64.0, dtype=np.float32)
