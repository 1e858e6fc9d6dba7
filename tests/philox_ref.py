"""numpy reference of the seeded noise stream (include/insv2v_hip.h, "seeded noise"): Philox4x32-10 words in uint64
arithmetic, uniforms and Box-Muller normals in float64.  A helper module of the seeded-noise tests, independent of the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or ints), key: 2 uint32 values -> 4 uint64 arrays holding the 32-bit output words."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in counter]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c


def _bits64(v):
    return int(v) & 0xFFFFFFFFFFFFFFFF       # an int64 as its two's-complement bits


def blocks(seed, stream, first_block, nblocks):
    """[nblocks, 4] uint32: blocks first_block ... first_block + nblocks - 1 of (seed, stream)."""
    seed, stream = _bits64(seed), _bits64(stream)
    b = np.uint64(first_block) + np.arange(nblocks, dtype=np.uint64)
    z = np.zeros(nblocks, dtype=np.uint64)
    out = philox4x32_10((b & MASK, b >> np.uint64(32), z + np.uint64(stream & 0xFFFFFFFF), z + np.uint64(stream >> 32)),
                        (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, 1).astype(np.uint32)


def words(seed, stream, offset, n):
    """uint32 [n]: elements [offset, offset + n) of the stream's raw words."""
    first = offset >> 2
    nb = ((offset + n + 3) >> 2) - first
    flat = blocks(seed, stream, first, max(nb, 0)).reshape(-1)
    return flat[offset - 4 * first:offset - 4 * first + n]


def normals(seed, stream, offset, n):
    """float64 [n]: elements [offset, offset + n) of the stream's normals."""
    first = offset >> 2
    nb = ((offset + n + 3) >> 2) - first
    w = blocks(seed, stream, first, max(nb, 0))
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    z = np.empty_like(u)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        z[:, a] = r * np.cos(2.0 * np.pi * u[:, a + 1])
        z[:, a + 1] = r * np.sin(2.0 * np.pi * u[:, a + 1])
    flat = z.reshape(-1)
    return flat[offset - 4 * first:offset - 4 * first + n]


def moments(z):
    """Sample statistics of the issue's table, in float64."""
    z = np.asarray(z, dtype=np.float64)
    m = z.mean()
    d = z - m
    var = (d * d).mean()
    lag = lambda k: float((d[:-k] * d[k:]).mean() / var)
    return {"mean": float(m), "var": float(var), "m3": float((z ** 3).mean()), "m4": float((z ** 4).mean()),
            "max": float(np.abs(z).max()), "lag1": lag(1), "lag4": lag(4)}


# (name, absolute bound): five standard errors at n = 2^20
MOMENT_BOUNDS = {"mean": (0.0, 5e-3), "var": (1.0, 7e-3), "m3": (0.0, 2e-2), "m4": (3.0, 5e-2), "lag1": (0.0, 5e-3), "lag4": (0.0, 5e-3)}


def check_moments(z):
    got = moments(z)
    for name, (centre, bound) in MOMENT_BOUNDS.items():
        assert abs(got[name] - centre) < bound, (name, got[name])
    return got
