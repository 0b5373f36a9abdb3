"""The G.711 contract in numpy (include/fastenhancer_hip.h, "Audio at another sample rate"): mu-law and A-law decode and encode written from
the contract's formulas - 32-bit ints, arithmetic shifts, hibit = the index of the highest set bit - and the four tables they give.  This
module imports nothing of the package: it is the oracle of fastenhancer_amd.g711 and of the resampler's G.711 instantiations."""
import hashlib

import numpy as np

LAWS = ("ulaw", "alaw")


def hibit(v):
    """index of the highest set bit of positive int32 values"""
    v = np.asarray(v, dtype=np.int32)
    assert (v > 0).all()
    h = np.zeros(v.shape, dtype=np.int32)
    for k in range(1, 31):
        h += v >= (1 << k)
    return h


def ulaw_dec(b):
    b = np.asarray(b).astype(np.int32)
    u = ~b & 0xFF
    e, m = (u >> 4) & 7, u & 15
    mag = (((m << 3) + 0x84) << e) - 0x84
    return np.where(u & 0x80, -mag, mag).astype(np.int16)


def alaw_dec(b):
    b = np.asarray(b).astype(np.int32)
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, mag, -mag).astype(np.int16)


def ulaw_enc(q):
    q = np.asarray(q).astype(np.int32)
    v = q >> 2
    neg = v < 0
    mask = np.where(neg, 0x7F, 0xFF)
    v = np.where(neg, -v, v)
    v = np.minimum(v, 8159) + 33
    seg = hibit(v) - 5
    t = np.where(seg >= 8, 0x7F, (seg << 4) | ((v >> (seg + 1)) & 15))
    return (t ^ mask).astype(np.uint8)


def alaw_enc(q):
    q = np.asarray(q).astype(np.int32)
    n = np.where(q >= 0, q, ~q)
    sign = np.where(q >= 0, 0x80, 0)
    small = n < 256
    e = np.where(small, 0, hibit(np.maximum(n, 256)) - 7)
    m = np.where(small, n >> 4, (n >> (e + 3)) & 15)
    return ((sign | (e << 4) | m) ^ 0x55).astype(np.uint8)


DEC = {"ulaw": ulaw_dec, "alaw": alaw_dec}
ENC = {"ulaw": ulaw_enc, "alaw": alaw_enc}


def dec(b, law):
    return DEC[law](b)


def enc(q, law):
    return ENC[law](q)


ALL_BYTES = np.arange(256, dtype=np.uint8)
ALL_SAMPLES = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)


def dec_table(law):
    """256 int16 values"""
    return dec(ALL_BYTES, law)


def enc_table(law):
    """65536 bytes, for q = -32768 .. 32767 in order"""
    return enc(ALL_SAMPLES, law)


def digest(table):
    """SHA-256, first 16 hex digits: int16 tables as little-endian, byte tables as they are"""
    t = np.asarray(table)
    return hashlib.sha256(t.astype("<i2").tobytes() if t.dtype == np.int16 else t.astype(np.uint8).tobytes()).hexdigest()[:16]


# the digests the contract states
DIGESTS = {("ulaw", "dec"): "3dab54339e520bb2", ("alaw", "dec"): "e04788d110e58ff8",
           ("ulaw", "enc"): "81d633c9e6972a18", ("alaw", "enc"): "38488f6fd710f468"}
DEC_RANGE = {"ulaw": 32124, "alaw": 32256}
MAX_ROUND_TRIP_ERROR = {"ulaw": 644, "alaw": 512}
ANCHORS = {"ulaw": {0: 0xFF, -1: 0x7E, 32767: 0x80, -32768: 0x00, 1000: 0xCE},
           "alaw": {0: 0xD5, -1: 0x55, 32767: 0xAA, -32768: 0x2A, 1000: 0xFA}}


def check_contract():
    """the digests, the anchors and the three properties of the contract; equality with CPython's audioop where it imports"""
    for law in LAWS:
        d, e = dec_table(law), enc_table(law)
        assert digest(d) == DIGESTS[(law, "dec")], (law, digest(d))
        assert digest(e) == DIGESTS[(law, "enc")], (law, digest(e))
        assert int(d.max()) == DEC_RANGE[law] and int(d.min()) == -DEC_RANGE[law]
        for q, b in ANCHORS[law].items():
            assert int(enc(np.array([q]), law)[0]) == b, (law, q)
        # enc(dec(b)) == b for every byte, but for mu-law's negative zero
        back = enc(d, law)
        differs = np.nonzero(back != ALL_BYTES)[0].tolist()
        assert differs == ([0x7F] if law == "ulaw" else []), (law, differs)
        if law == "ulaw":
            assert int(d[0xFF]) == 0 and int(d[0x7F]) == 0 and int(back[0x7F]) == 0xFF
        # dec(enc(q)) is non-decreasing in q, and never further from q than the law's largest step allows
        rt = dec(e, law).astype(np.int32)
        assert (np.diff(rt) >= 0).all(), law
        assert int(np.abs(rt - ALL_SAMPLES.astype(np.int32)).max()) == MAX_ROUND_TRIP_ERROR[law], law
    try:
        import audioop
    except ImportError:         # (removed from CPython 3.13: the formulas and the digests stand without it)
        return False
    for law, to_lin, from_lin in (("ulaw", audioop.ulaw2lin, audioop.lin2ulaw), ("alaw", audioop.alaw2lin, audioop.lin2alaw)):
        assert np.frombuffer(to_lin(ALL_BYTES.tobytes(), 2), dtype=np.int16).tolist() == dec_table(law).tolist(), law
        assert np.frombuffer(from_lin(ALL_SAMPLES.astype("<i2").tobytes(), 2), dtype=np.uint8).tolist() == enc_table(law).tolist(), law
    return True
