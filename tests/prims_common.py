"""Shared by tests/test_prims_cpu.py and tests/test_gpu_prims.py: exact numpy references of the shared device primitives (csrc/radix_sort.h, the
sort half of csrc/cell_list.h, the union-find of csrc/union_find.h), the key generators and case tables the GPU tests run, and checkers that
compare bit for bit.  Plain numpy, no GPU; nothing here is imported by the product.  All of it is integer work: no tolerance anywhere."""
import numpy as np

TILE = 2048                                                        # RS_TILE and SCB_TILE: the elements one workgroup of the sort / the tiled scan takes
SENTINEL = 0xA5                                                    # every output byte before a call
WS_FILL = 0x55                                                     # every workspace byte before a call
INT32_MIN = -(1 << 31)


def cdiv(a, b):
    return (a + b - 1) // b


def sorted_bits(bits):
    """The key bits the sort orders by: whole 8-bit digits, [0, 8 * ceil(bits / 8))."""
    return 8 * cdiv(bits, 8)


def sort_mask(bits):
    return np.uint64((1 << sorted_bits(bits)) - 1)


def bits_for(maxkey):
    """csrc/radix_sort.h bits_for: the bits needed to write maxkey."""
    return int(maxkey).bit_length()


# ---- references
def sort_order(keys, bits):
    keys = np.asarray(keys, np.uint64)
    if bits == 0:
        return np.arange(len(keys))
    return np.argsort(keys & sort_mask(bits), kind='stable')


def ref_sort(keys, vals, bits):
    """(keys_out, vals_out) of a stable sort by the bits [0, 8 * ceil(bits / 8)); the whole 64-bit keys come out, permuted."""
    order = sort_order(keys, bits)
    return np.asarray(keys, np.uint64)[order], np.asarray(vals, np.int32)[order]


def ref_cell_starts(sorted_keys, nc):
    """cstart[c] = the first sorted position whose key is >= c, c = 0 .. nc."""
    return np.searchsorted(np.asarray(sorted_keys, np.uint64), np.arange(nc + 1, dtype=np.uint64), 'left').astype(np.int32)


def ref_sort_by_cell(keys, nc):
    """(sorted keys, the points' indices in that order = the stable argsort of keys, cstart [nc + 1]) as sort_by_cell leaves them."""
    keys = np.asarray(keys, np.uint64)
    order = sort_order(keys, bits_for(nc))
    return keys[order], order.astype(np.int32), ref_cell_starts(keys[order], nc)


def ref_scan(x, inclusive):
    """int32 -> int32 (summed in int64; the sum must fit, as the header requires), uint64 -> uint64 modulo 2^64."""
    x = np.asarray(x)
    if x.dtype == np.uint64:
        inc = np.cumsum(x, dtype=np.uint64)
    else:
        assert x.dtype == np.int32, x.dtype
        inc = np.cumsum(x, dtype=np.int64)
        assert inc.min(initial=0) >= INT32_MIN and inc.max(initial=0) < (1 << 31), "the case's sum does not fit an int"
    out = inc if inclusive else np.concatenate([np.zeros(1, inc.dtype), inc[:-1]])
    return out.astype(x.dtype)


# ---- checkers
def check_equal(got, want, what):
    """Bit for bit; on a mismatch: the first differing index, its tile and its position inside the tile."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ; the first at index {i} (tile {i // TILE}, position {i % TILE}): "
                         f"got {got[i]!r} ({int(got[i]) & (2 ** 64 - 1):#x}), expected {want[i]!r} ({int(want[i]) & (2 ** 64 - 1):#x})")


def check_sort(keys, vals, bits, keys_out, vals_out):
    k, v = ref_sort(keys, vals, bits)
    check_equal(keys_out, k, f"radix_sort keys (n={len(k)}, bits={bits})")
    check_equal(vals_out, v, f"radix_sort values (n={len(k)}, bits={bits})")


def check_sort_by_cell(keys, nc, keys_out, idx_out, cstart_out):
    k, i, c = ref_sort_by_cell(keys, nc)
    check_equal(keys_out, k, f"sort_by_cell keys (n={len(k)}, nc={nc})")
    check_equal(idx_out, i, f"sort_by_cell indices (n={len(k)}, nc={nc})")
    check_equal(cstart_out, c, f"k_cell_starts (n={len(k)}, nc={nc})")


def check_scan(x, inclusive, out):
    check_equal(out, ref_scan(x, inclusive), f"{'inclusive' if inclusive else 'exclusive'} {np.asarray(x).dtype} scan (n={len(x)})")


# ---- key generators: gen_keys(name, n, bits, seed) -> uint64 [n], keys < 2^bits unless the generator says otherwise
def _rand(rng, bits, size):
    if bits == 0:
        return np.zeros(size, np.uint64)
    return rng.integers(0, 1 << bits, size, dtype=np.uint64)


def _uniform(rng, n, bits):
    return _rand(rng, bits, n)


def _equal(rng, n, bits):
    return np.repeat(_rand(rng, bits, 1), n)


def _two_values(rng, n, bits):
    a, b = _rand(rng, bits, 2)
    if a == b and bits > 0:
        b = a ^ np.uint64(1)
    return np.where(rng.random(n) < 0.9, a, b).astype(np.uint64)


def _sorted(rng, n, bits):
    return np.sort(_rand(rng, bits, n))


def _reversed(rng, n, bits):
    return np.sort(_rand(rng, bits, n))[::-1].copy()


def _top_byte_only(rng, n, bits):
    """One fixed pattern in the digits below the highest used one; that digit (bits - 8 d wide, d its index) random."""
    d = max(bits - 1, 0) // 8
    low = _rand(rng, 8 * d, 1)[0]
    return (_rand(rng, bits - 8 * d, n) << np.uint64(8 * d)) | low


def _digits_0_255(rng, n, bits):
    """Every digit 0 or 255 (the partial top digit: 0 or all its bits)."""
    k = np.zeros(n, np.uint64)
    for d in range(cdiv(bits, 8)):
        k |= (rng.integers(0, 2, n).astype(np.uint64) * np.uint64(255)) << np.uint64(8 * d)
    return k & np.uint64((1 << bits) - 1)


def _wave_uniform(rng, n, bits):
    """Runs of 64 equal keys aligned to 64: all 64 lanes of a wave carry one digit in every pass."""
    return np.repeat(_rand(rng, bits, cdiv(n, 64)), 64)[:n].copy()


def _wave_distinct(rng, n, bits):
    """Within each aligned 64 the low digit is a permutation of 64 distinct values: no two lanes of a wave share a digit in the first pass."""
    assert bits >= 8
    low = np.concatenate([rng.permutation(256)[:64] for _ in range(cdiv(n, 64))])[:n].astype(np.uint64)
    return (_rand(rng, bits, n) & ~np.uint64(255)) | low


def _above_bits(rng, n, bits):
    """Keys < 2^bits with random bits set on top: in [bits, 8 * ceil(bits / 8)), which take part in the order, and in [8 * ceil(bits / 8), 64),
    which do not.  Both sets must come out intact."""
    sb = sorted_bits(bits)
    k = _rand(rng, bits, n)
    if sb > bits:
        k |= _rand(rng, sb - bits, n) << np.uint64(bits)
    if sb < 64:
        k |= _rand(rng, 64 - sb, n) << np.uint64(sb)
    return k


GENERATORS = {'uniform': _uniform, 'equal': _equal, 'two_values': _two_values, 'sorted': _sorted, 'reversed': _reversed,
              'top_byte_only': _top_byte_only, 'digits_0_255': _digits_0_255, 'wave_uniform': _wave_uniform, 'wave_distinct': _wave_distinct,
              'above_bits': _above_bits}


def _seed(*parts):
    return [int(p) if not isinstance(p, str) else sum(ord(c) * 131 ** i for i, c in enumerate(p)) % (1 << 31) for p in parts]


def gen_keys(name, n, bits, seed=0):
    k = GENERATORS[name](np.random.default_rng(_seed(name, n, bits, seed)), n, bits)
    assert k.dtype == np.uint64 and k.shape == (n,)
    return k


def gen_vals(keys, bits, seed=0):
    """A random permutation of 0 .. n - 1 as int32, except that the slots of two keys that occur more than once (under the sorted bits) hold
    INT32_MIN and -1: values whose sign bit must survive, on keys whose order only stability decides.  Where no key repeats, the first and the last
    slot take them."""
    n = len(keys)
    rng = np.random.default_rng(_seed('vals', n, bits, seed))
    vals = rng.permutation(n).astype(np.int32)
    masked = np.asarray(keys, np.uint64) & (sort_mask(bits) if bits else np.uint64(0))
    uniq, inverse, counts = np.unique(masked, return_inverse=True, return_counts=True)
    dup = np.flatnonzero(counts[inverse.reshape(-1)] > 1)
    slots = rng.choice(dup, 2, replace=False) if len(dup) >= 2 else np.array([0, n - 1])
    vals[slots[0]] = INT32_MIN
    if slots[1] != slots[0]:
        vals[slots[1]] = -1
    return vals


# ---- cell keys: cell_keys(name, n, nc, seed) -> uint64 [n]
CELL_SETS = ('uniform', 'first', 'last', 'third_empty', 'outside')


def cell_keys(name, n, nc, seed=0):
    rng = np.random.default_rng(_seed('cells', name, n, nc, seed))
    if name == 'uniform':
        k = rng.integers(0, nc, n)
    elif name == 'first':
        k = np.zeros(n, np.int64)
    elif name == 'last':
        k = np.full(n, nc - 1, np.int64)
    elif name == 'third_empty':                                     # the cells 2, 5, 8, ... stay empty
        cells = np.arange(nc)
        cells = cells[cells % 3 != 2]
        k = cells[rng.integers(0, len(cells), n)]
    elif name == 'outside':                                         # a tenth of the keys equal to nc, as mesh_distance.hip keys the faces it drops
        assert nc > 1
        k = np.where(rng.random(n) < 0.1, nc, rng.integers(0, nc, n))
    else:
        raise KeyError(name)
    return np.asarray(k).astype(np.uint64)


# ---- the case tables of tests/test_gpu_prims.py
SORT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4097, 11017, 300001)
SORT_BITS = (0, 1, 7, 8, 9, 16, 19, 25, 45, 63, 64)
SORT_CASES = ([(g, n, 33) for n in SORT_SIZES for g in ('uniform', 'two_values')]              # sizes
              + [('uniform', 4097, b) for b in SORT_BITS]                                       # key widths
              + [(g, 11017, b) for g in GENERATORS for b in (19, 45)])                          # every generator, a partial and a later top digit
CELL_SHAPES = ((1, 1), (2049, 1), (2049, 7), (4097, 300), (11017, 70000), (11017, 65536))
CELL_CASES = [(s, n, nc) for n, nc in CELL_SHAPES for s in CELL_SETS if not (s == 'outside' and nc == 1)]
KSCAN_SIZES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 37893)
TILED_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 6145, 2048 * 1024, 2048 * 1025 + 3)
TILED_LARGE = TILED_SIZES[-2:]                                     # nt == SC_T and nt == SC_T + 1: (int, exclusive) and (uint64_t, inclusive) only
SCAN_FORMS = (('int', 0), ('int', 1), ('uint64', 0), ('uint64', 1))                             # (element type, inclusive)


# ---- the union-find of csrc/union_find.h: union_case(name) -> (n, pairs int32 [P, 2]); the reference is mesh_clean_common.union_find
UNION_N = 4096                                                     # 16 workgroups of 256 pairs; a chain of it gives the longest walks there are
UNION_CASES = ('single', 'self_pair', 'chain_ascending', 'chain_descending', 'chain_shuffled', 'star_on_first', 'star_on_last', 'chain_four_times',
               'random_3000_on_1000', 'pairs_255', 'pairs_256', 'pairs_257')


def union_case(name):
    rng = np.random.default_rng(_seed('union', name))
    n = UNION_N
    i = np.arange(n - 1)
    chain = np.stack([i, i + 1], 1)
    if name == 'single':
        n, p = 1, np.zeros((0, 2))
    elif name == 'self_pair':
        n, p = 1, np.zeros((1, 2))
    elif name == 'chain_ascending':
        p = chain
    elif name == 'chain_descending':
        p = chain[::-1]
    elif name == 'chain_shuffled':
        p = chain[rng.permutation(n - 1)]
    elif name == 'star_on_first':                                   # every thread's CAS meets the one root
        p = np.stack([np.zeros(n - 1, np.int64), i + 1], 1)
    elif name == 'star_on_last':
        p = np.stack([np.full(n - 1, n - 1), i], 1)
    elif name == 'chain_four_times':                                # every pair listed four times, both ways round
        p = np.concatenate([chain, chain[:, ::-1], chain, chain[:, ::-1]])[rng.permutation(4 * (n - 1))]
    elif name == 'random_3000_on_1000':
        n, p = 1000, rng.integers(0, 1000, (3000, 2))
    elif name.startswith('pairs_'):                                 # the workgroup edge of the one-thread-per-pair launch
        n, p = 600, rng.integers(0, 600, (int(name[6:]), 2))
    else:
        raise KeyError(name)
    return n, np.ascontiguousarray(p).astype(np.int32)


def ref_union(n, pairs):
    """root [n] int32: the smallest index of every class (a sequential union-find, the smaller index staying the root)."""
    from mesh_clean_common import union_find
    return union_find(n, pairs)


def scan_inputs(elem, n, tiled):
    """{name: input array} of one scan case.  int: zeros and ones (k_scan), random 0 .. 3, and (tiled) 0 / 1 flags that are 1 only at the first and
    the last element of every tile; uint64_t: random < 2^40 (the sum passes 2^32 inside the second tile), and at n = 6145 of the tiled scan every
    element 2^32 - 1."""
    rng = np.random.default_rng(_seed('scan', elem, n, int(tiled)))
    if elem == 'int':
        d = {'random_0_3': rng.integers(0, 4, n).astype(np.int32)}
        if tiled:
            f = np.zeros(n, np.int32)
            f[0::TILE] = 1
            f[TILE - 1::TILE] = 1
            f[n - 1] = 1                                            # (the last tile's last element too, where that tile is ragged)
            d['tile_edge_flags'] = f
        else:
            d['zeros'], d['ones'] = np.zeros(n, np.int32), np.ones(n, np.int32)
        return d
    d = {'random_2_40': rng.integers(0, 1 << 40, n, dtype=np.uint64)}
    if tiled and n == 6145:
        d['all_2_32_minus_1'] = np.full(n, (1 << 32) - 1, np.uint64)
    return d
