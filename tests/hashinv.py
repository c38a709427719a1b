"""Inverses of the two device hashes (csrc/phj_hash.h), test infrastructure.

Both XXH3's 8-byte path and Murmur3's fmix64 are bijections of the 64-bit
keys; these step-by-step inverses prove it (tests/test_hash_codes.py) and turn
a chosen hash code into the key that has it (preimage keys planted by the GPU
parity tests: codes equal to a code table's empty value E_p, csrc/phj_table.h;
keys crowded into one LDS bucket or homed at the NoPartitioning table's edges
for the row joins, tests/test_gpu_collisions.py), with numpy restatements of
where a code goes: its partition, its LDS bucket, its NoPartitioning home.
"""
import numpy as np

M64 = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _inv_xorshift_right(y, s):
    # x ^= x >> s
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def _inv_mul(c):
    return pow(c, -1, 1 << 64)


def _xxh3_bitflip(seed):
    s = seed & 0xFFFFFFFF
    swapped = int.from_bytes(s.to_bytes(4, "little"), "big")
    seed ^= swapped << 32
    return ((0x1CAD21F72C81017C ^ 0xDB979083E96DD4DE) - seed) & M64


def _inv_lin(y):
    # x ^ rotl(x,49) ^ rotl(x,24) is linear over GF(2): invert by Gaussian
    # elimination on its 64 column images
    cols = []
    for i in range(64):
        e = 1 << i
        cols.append(e ^ _rotl(e, 49) ^ _rotl(e, 24))
    # solve A x = y: rows = output bits
    rows = []
    for bit in range(64):
        r = 0
        for i in range(64):
            if (cols[i] >> bit) & 1:
                r |= 1 << i
        rows.append([r, (y >> bit) & 1])
    piv = []
    rank = 0
    for col in range(64):
        sel = next((j for j in range(rank, 64) if (rows[j][0] >> col) & 1), None)
        assert sel is not None, "linear mixer not invertible"
        rows[rank], rows[sel] = rows[sel], rows[rank]
        for j in range(64):
            if j != rank and (rows[j][0] >> col) & 1:
                rows[j][0] ^= rows[rank][0]
                rows[j][1] ^= rows[rank][1]
        piv.append(col)
        rank += 1
    x = 0
    for j, col in enumerate(piv):
        x |= rows[j][1] << col
    return x


def xxh3_inverse(h, seed):
    C = 0x9FB21C651E98DF25
    x = _inv_xorshift_right(h, 28)
    x = (x * _inv_mul(C)) & M64
    # y = x ^ ((x >> 35) + 8): bits 30..63 of x pass through unchanged
    hi = x >> 35
    x = x ^ ((hi + 8) & M64)
    x = (x * _inv_mul(C)) & M64
    x = _inv_lin(x)
    x ^= _xxh3_bitflip(seed)
    return ((x >> 32) | (x << 32)) & M64


def murmur3_inverse(h, seed):
    x = _inv_xorshift_right(h, 33)
    x = (x * _inv_mul(0xC4CEB9FE1A85EC53)) & M64
    x = _inv_xorshift_right(x, 33)
    x = (x * _inv_mul(0xFF51AFD7ED558CCD)) & M64
    x = _inv_xorshift_right(x, 33)
    return x ^ seed



def preimage(kind_is_murmur3, code, seed):
    """The int64 key whose hash code is `code` (uint64)."""
    u = (murmur3_inverse if kind_is_murmur3 else xxh3_inverse)(code & M64, seed & M64)
    return int(np.array([u], dtype=np.uint64).view(np.int64)[0])


_HASH_MURMUR3 = 1   # include/phj.h PHJ_HASH_MURMUR3


def _keys_of(params, codes):
    """The distinct int64 keys whose codes under params' hash and seed are `codes`."""
    mur = params.hash == _HASH_MURMUR3
    keys = np.array([preimage(mur, c, params.hash_seed) for c in codes], dtype=np.int64)
    assert len(np.unique(keys)) == len(codes)
    return keys


def odd_part(num_partitions):
    """num_partitions with its factors of two removed (1 for radix bits)."""
    m = num_partitions if num_partitions > 0 else 1
    while m % 2 == 0:
        m //= 2
    return m


def partition_mates(params, n, base=0):
    """n distinct keys of one final partition and one LDS bucket whatever the
    plan's refinement: their codes are base + t L, t = 0 .. n - 1, with
    L = 2^50 odd(P). P <= 2^22 divides L, so the codes share h % P; they share
    h's low 50 bits, so every h & (2^k - 1), the sub-partition bits above the
    radix bits or from bit 40 on (up to ten of those), and bits 32..49, the
    LDS bucket (h >> 32) & (nbk - 1) at every round size. t odd(P) < 2^14
    keeps the codes below 2^64; more mates than that allows is an error."""
    m = odd_part(params.num_partitions)
    if not 0 <= base < (1 << 50):
        raise ValueError("base must be below 2^50")
    if n < 0 or (n > 0 and (n - 1) * m >= (1 << 14)):
        raise ValueError(f"at most {((1 << 14) - 1) // m + 1} mates with odd(P) = {m}")
    return _keys_of(params, [base + ((t * m) << 50) for t in range(n)])


NP_EDGES = {   # where: (high word of the code, low 22 bits)
    "last_of_table": (0xFFFFFFFF, (1 << 22) - 1),
    "last_of_region0": (0xFFFFFFFF, 0),
    "first_of_table": (0, 0),
    "first_of_region1": (0, 1),
}


def np_edge_keys(params, where, n):
    """n <= 1024 distinct keys at an edge of the NoPartitioning table
    (csrc/phj_join.h np_home_r: region = the code's low rbits, rbits <= 22;
    home bucket inside it = (high word * nbr) >> 32). High word 2^32 - 1: the
    region's last bucket for every nbr; 0: its first. Low 22 bits all ones:
    the last region for every rbits; 0: region 0; 1: region 1 for every
    rbits >= 1 (the build always makes at least two regions). Bits 22..31
    count the keys, so none of this needs the table's geometry."""
    hi, low = NP_EDGES[where]
    if not 0 <= n <= 1024:
        raise ValueError("at most 1024 keys: the counter is bits 22..31")
    return _keys_of(params, [(hi << 32) | (t << 22) | low for t in range(n)])


def partition_of(codes, params, sub_bits=0):
    """csrc/phj_partition.h q_from_hash over uint64 codes: h & (2^k - 1) for
    radix bits, h % P otherwise; refined by sub_bits further bits (the bits
    just above the radix bits, or from bit 40 on: csrc/phj_capi.hip
    refine_plan)."""
    codes = np.asarray(codes, dtype=np.uint64)
    one = np.uint64(1)
    if params.num_partitions > 0:
        q, shift = codes % np.uint64(params.num_partitions), 40
    else:
        shift = int(params.radix_bits[0]) + int(params.radix_bits[1])
        q = codes & ((one << np.uint64(shift)) - one)
    if sub_bits:
        q = (q << np.uint64(sub_bits)) | ((codes >> np.uint64(shift)) & ((one << np.uint64(sub_bits)) - one))
    return q


def lds_bucket(codes, nbk=128):
    """csrc/phj_join.h bucket_of: the LDS table's bucket, nbk a power of two <= 128."""
    return (np.asarray(codes, dtype=np.uint64) >> np.uint64(32)) & np.uint64(nbk - 1)


def np_geometry(n_build, table_ratio):
    """(nb, nbr, rbits) of the NoPartitioning table over n_build tuples
    (csrc/phj_capi.hip np_build; table_ratio 0 is the default 2.0): 2^rbits
    regions of nbr buckets of 7 slots, at least two regions of at most 1024."""
    ratio = table_ratio if table_ratio > 0 else 2.0
    nb0 = max(1, int(np.ceil(n_build * ratio / 7)))
    want = (nb0 + 1023) // 1024
    rbits = min(22, max(1, (want - 1).bit_length()))
    nbr = (nb0 + (1 << rbits) - 1) >> rbits
    return nbr << rbits, nbr, rbits


def np_home(codes, geometry):
    """csrc/phj_join.h np_home_r: region = the low rbits, bucket inside it from the high word."""
    nb, nbr, rbits = geometry
    codes = np.asarray(codes, dtype=np.uint64)
    r = codes & np.uint64((1 << rbits) - 1)
    return r * np.uint64(nbr) + (((codes >> np.uint64(32)) * np.uint64(nbr)) >> np.uint64(32))


def table_edge_codes(num_partitions):
    """Codes at the code tables' edges (csrc/phj_table.h, csrc/phj_cluster.h): 0, 1 and 2^40 (the
    empty values E_p of every plan: E_p = 0 for p != 0, E_0 = 1, or 2^40 under
    h % 1), 2, 3, 2^64 - 1, and "bucket mates" of 0, 1 and 2^40: codes of the
    same final partition and the same home bucket ((c >> 24) & mask = 0),
    c + (m t) << 50 with m = P for h % P (the residue mod P is kept while
    m t < 2^14) and m = 1 for radix bits and NoPartitioning regions (low bits
    kept). Planted in R they fill the bucket an E-coloured slot sits in, so a
    slot mistaken for empty ends other codes' walks early."""
    m = num_partitions if num_partitions > 0 else 1
    ts = [t for t in range(1, 9) if m * t < (1 << 14)]
    codes = {0, 1, 2, 3, 1 << 40, M64}
    for b in (0, 1, 1 << 40):
        for t in ts:
            codes.add(b + ((m * t) << 50))
    # the LDS join's cluster tables (csrc/phj_cluster.h): E of cluster 0 is the
    # plan's lowest power of two outside cluster 0 (2^(log2 P - k) for radix
    # bits, 2^40.. under h % P with sub-partition bits): every power of two,
    # and bucket mates of those a cluster plan can pick
    for b in range(64):
        codes.add(1 << b)
    for b in list(range(0, 17)) + [40, 41, 42]:
        for t in ts[:3]:
            codes.add((1 << b) + ((m * t) << 50))
    return sorted(c & M64 for c in codes)
