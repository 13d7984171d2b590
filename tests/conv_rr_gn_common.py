"""Shared by tests/test_gpu_conv_rr_gn.py and tests/test_conv_rr_gn_cpu.py: the case grid of k_conv_rr's in-staging GroupNorm (csrc/nn_conv_rr.hip), the octet
partials the tests hand it, the statistics those partials imply, the float64 reference with its per-element bound (tests/nn_ops_common.py: the bound the
stand-alone k_gn_apply already passes -- no tolerance of this file's own), and a torch emulation of the staged element map with the mistakes the
statistics code of such a kernel can make.  Plain torch, device-agnostic, nothing imported from the product.

The probe.  A 1x1 conv (taps = 1) with Cout = C, the f16 identity as weights, no bias and no residual: every output is one product 1.0 * t plus exact
zeros in f32, so y[n, p, c] is exactly the f16 value t the kernel staged for (n, p, c) -- the staged element map, without conv arithmetic in the way.

The partials.  [N][chunks][C / 8][2] float32 (sum, sum of squares) per source, over an arbitrary uneven split of the pixels into `chunks` runs (some may be
empty): the kernel only sums what it is given, so chunk counts need not divide H * W.  pps = max(1, 256 / (C / 8)) slots (C: the whole, possibly two-source,
input) each take chunks sl, sl + pps, ...; the host accepts at most 8 per slot, i.e. 8 pps chunks per source.

The statistics.  implied_stats() combines the partials in float64, as the kernel does; what is left between the two is the order of a float64 sum of at
most 512 float32 slots (512 * 2^-53 = 2^-20 of an f32 roundoff: STATS_TERMS) and the f32 rounding of mean and rstd, which gn_stats_bounds adds.

The grid.  Image = the variant's own width squared, N = 2 (a wrong per-image partial offset shows).  Variants with the in-staging path: 1, 2, 3, 5.
Single-source C in {256 ... 2048}: every multiple of the unit size with a group size that is a multiple of 8, up to the host's limit; 768 and 1536 give
groups that straddle unit boundaries; (variant 1, 256) is the unit with 32 groups.  Two-source splits with chunksA != chunksB; (512, 256) and (1024, 512)
put a group across the A | B boundary.  Chunk classes, gn_mode 1 / 2, FiLM on / off (rows differ per image), one slab / as many slabs as units: the product
is pruned to three cases per (variant, channel configuration), rotated so that every class occurs with every variant (tests/test_conv_rr_gn_cpu.py counts
them), and (variant 1, 256) gets every chunk class."""
import torch

import nn_ops_common as oc

N_IMG = 2
VARIANTS = {1: (8, 256), 2: (16, 128), 3: (32, 128), 5: (8, 128)}          # id -> (image width, channels per staged unit): rr_variant(), nn_conv_rr.hip
SINGLE_C = (256, 512, 768, 1024, 1536, 2048)
TWO_SOURCE = ((256, 256), (512, 256), (1024, 512))
CHUNK_CLASSES = ('one', 'pps-1', 'pps', 'pps+1', 'odd', 'max')
MAX_PART_LOADS = 8                                                        # PD_RR_MAX_PART_LOADS
STATS_TERMS = 2.0 ** -20
# the UNet of the engine case: the smallest whose 8^2 level has 256 channels (32^2 input, 64 base channels, multipliers 1, 2, 4, one ResBlock per level)
ENGINE_CFG = dict(image_size=32, num_channels=64, num_res_blocks=1, attention_resolutions="8", num_head_channels=64, channel_mult="1,2,4")


def pps_of(C):
    return max(1, 256 // (C // 8))


def chunk_count(cls, C):
    """Chunks per image of class `cls` for a C-channel (whole) input; None where the class does not exist (pps - 1 == 0)."""
    pps = pps_of(C)
    n = {'one': 1, 'pps-1': pps - 1, 'pps': pps, 'pps+1': pps + 1, 'odd': 4 * pps + 1 + 2 * (pps > 1), 'max': MAX_PART_LOADS * pps,
         'over': MAX_PART_LOADS * pps + 1}[cls]
    return n if n >= 1 else None


def unit_groups(cs, C):
    """The kernel's own group count per staged unit (issue_stats: g_first = (c0 * mg) >> 20, ng = (((c0 + CS - 1) * mg) >> 20) - g_first + 1), every unit."""
    cg = C // 32
    mg = ((1 << 20) + cg - 1) // cg
    return [(((c0 + cs - 1) * mg) >> 20) - ((c0 * mg) >> 20) + 1 for c0 in range(0, C, cs)]


def _cases():
    cases = []
    for vi, (v, (W, cs)) in enumerate(VARIANTS.items()):
        configs = [(C, 0) for C in SINGLE_C] + list(TWO_SOURCE)
        for ci, (Ca, Cb) in enumerate(configs):
            C = Ca + Cb
            if (v, Ca, Cb) == (1, 256, 0):
                classes = list(CHUNK_CLASSES)
            else:
                classes = [CHUNK_CLASSES[(ci + vi + 2 * k) % 6] for k in range(3)]
            seen = set()
            for k, cls in enumerate(classes):
                chA = chunk_count(cls, C)
                if chA is None or chA in seen:
                    continue
                seen.add(chA)
                chB = 0
                if Cb:
                    nxt = [c for c in (chunk_count(o, C) for o in CHUNK_CLASSES[CHUNK_CLASSES.index(cls) + 1:] + CHUNK_CLASSES) if c and c != chA]
                    chB = nxt[0]
                units = C // cs
                many = (k + ci + vi) % 2 == 0 and units > 1
                cg = C // 32
                cases.append(dict(
                    name=f"v{v}-{Ca}+{Cb}-{cls}{chA}" + (f"|{chB}" if Cb else "") + f"-gn{1 + (k + ci) % 2}" + ("-film" if (k + ci // 2 + vi) % 2 else "") +
                         (f"-slabs{units}" if many else ""),
                    variant=v, W=W, cs=cs, Ca=Ca, Cb=Cb, C=C, cls=cls, chunksA=chA, chunksB=chB, mode=1 + (k + ci) % 2, film=bool((k + ci // 2 + vi) % 2),
                    slabs=units if many else 1, groups_max=max(unit_groups(cs, C)),
                    straddles_unit=cs % cg != 0,                  # a group lies across two staged units
                    straddles_ab=bool(Cb) and Ca % cg != 0))      # a group lies across the A | B boundary
    return cases


CASES = _cases()


def _refusals():
    """(name, variant, Ca, Cb, chunksA, chunksB, message): one chunk more than the host accepts, per source, and a group size that is no multiple of 8 (1152 / 32 = 36;
    no multiple of variant 1's 256-channel unit has such a group size, so variant 1 has no such case)."""
    out = []
    for v, (W, cs) in VARIANTS.items():
        C = {1: 256, 2: 1024, 3: 2048, 5: 512}[v]
        out.append((f"v{v}-{C}-over", v, C, 0, chunk_count('over', C), 0, b"outside the in-kernel statistics' range"))
        out.append((f"v{v}-512+256-overB", v, 512, 256, 1, chunk_count('over', 768), b"outside the in-kernel statistics' range"))
        if 1152 % cs == 0:
            out.append((f"v{v}-1152-group36", v, 1152, 0, 1, 0, b"group size that is a multiple of 8"))
    return out


REFUSALS = _refusals()

# the two rows added to CASES of tests/test_gpu_round6.py: variant 0 = the automatic selection of pdhip_conv_rr_f16 (8^2, 256 channels: variant 1's 32-group unit)
ROUND6_ROWS = [(1, 8, 256, 0, 512, 1, False, None, 0, 1, 0, 0, 0), (1, 8, 256, 0, 512, 2, True, None, 0, 1, 0, 0, 0)]


def inputs(c, seed=0):
    """x [N, W, W, C] f16, gamma, beta [C] f32, film [N, 2 C] f32 (rows differ per image) of a case: nn_ops_common.gn_inputs."""
    return oc.gn_inputs(N_IMG, c['W'], c['W'], c['C'], seed)


def chunk_bounds(HW, chunks, seed):
    """chunks + 1 non-decreasing pixel indices 0 ... HW: an uneven split (empty runs allowed: a producer may leave a zero partial)."""
    g = torch.Generator().manual_seed(7919 * HW + 31 * chunks + seed)
    cuts = sorted(torch.randint(0, HW + 1, (chunks - 1,), generator=g).tolist())
    return [0] + cuts + [HW]


def octet_partials(x, chunks, seed=0):
    """x [N, H, W, Cx] f16 (one source) -> [N, chunks, Cx / 8, 2] float32 on x's device: per run of chunk_bounds the f32 (sum, sum of squares) of every octet."""
    N, Cx = x.shape[0], x.shape[-1]
    v = x.float().reshape(N, -1, Cx // 8, 8)
    b = chunk_bounds(v.shape[1], chunks, seed)
    out = torch.zeros((N, chunks, Cx // 8, 2), dtype=torch.float32, device=x.device)
    for c in range(chunks):
        if b[c + 1] > b[c]:
            r = v[:, b[c]:b[c + 1]]
            out[:, c, :, 0] = r.sum(dim=(1, 3))
            out[:, c, :, 1] = (r * r).sum(dim=(1, 3))
    return out


def case_partials(c, x):
    """(partA, partB or None) of a case: the sources are chunked differently and split differently."""
    pa = octet_partials(x[..., :c['Ca']], c['chunksA'], 1)
    pb = octet_partials(x[..., c['Ca']:], c['chunksB'], 2) if c['Cb'] else None
    return pa, pb


def implied_stats(parts, HW):
    """parts: the [N, chunks_i, C_i / 8, 2] partials of the sources in concat order -> float64 (mean, rstd) [N, 32] of GroupNorm(32) over the concat."""
    octs = torch.cat([p.double().sum(dim=1) for p in parts], dim=1)             # [N, octets, 2]
    N, O = octs.shape[:2]
    g = octs.reshape(N, 32, O // 32, 2).sum(dim=2)
    cnt = HW * (O // 32) * 8
    mean = g[..., 0] / cnt
    var = (g[..., 1] / cnt - mean * mean).clamp(min=0)
    return mean, (var + oc.EPS) ** -0.5


def reference(x, gamma, beta, film, mode, mean, rstd):
    """(reference, bound) [N, H, W, C] float64 of the staged map given the statistics the partials imply: nn_ops_common.gn_ref under gn_stats_bounds."""
    dm, dr = oc.gn_stats_bounds(x, STATS_TERMS)
    return oc.gn_ref(x, gamma, beta, film, 1 if mode == 2 else 0, 0, mean, rstd, dm, dr)


# ================================================================================================ emulation (CPU test)
def kernel_stats(parts, Cs, HW, mistake=None, at=(1, 0)):
    """(mean, rstd) [N, 32] float32 the way the kernel finishes them: slot (octet k of the group, sl) sums chunks sl, sl + pps, ... of its source in f64, the
    group adds its opg x pps slots, mean / rstd are rounded to f32.  parts / Cs: one or two sources.  mistake, applied at (image, group) = at:
      'drop_last_chunk'  slot 0 of the group's first octet leaves out its last chunk
      'image0'           the partials of image 0 are read for image `at[0]` (a missing per-image offset)
      'chunks_of_b'      the group's octets in source A are read with source B's chunk count (count and per-image stride)
      'zero_mean' / 'neighbour'   the finished mean is zero / both statistics are those of group at[1] + 1"""
    C = sum(Cs)
    N = parts[0].shape[0]
    opg, pps, oa = C // 32 // 8, pps_of(C), Cs[0] // 8
    flat = [p.double().reshape(-1, 2) for p in parts]                          # [(n * chunks + c) * os + o]
    chunks = [p.shape[1] for p in parts]
    sums = torch.zeros((N, 32, 2), dtype=torch.float64)
    for n in range(N):
        for g in range(32):
            hit = mistake is not None and (n, g) == tuple(at)
            for k in range(opg):
                o = g * opg + k
                src = 0 if o < oa else 1
                ch, os_, ol = chunks[src], Cs[src] // 8, o if o < oa else o - oa
                img = n
                if hit and mistake == 'chunks_of_b' and src == 0:
                    ch = chunks[1]
                if hit and mistake == 'image0':
                    img = 0
                for sl in range(pps):
                    idx = list(range(sl, ch, pps))
                    if hit and mistake == 'drop_last_chunk' and k == 0 and sl == 0:
                        idx = idx[:-1]
                    for cc in idx:
                        sums[n, g] += flat[src][(img * ch + cc) * os_ + ol]
    cnt = HW * (C // 32)
    mean = sums[..., 0] / cnt
    var = (sums[..., 1] / cnt - mean * mean).clamp(min=0)
    mean, rstd = mean.float(), ((var + oc.EPS) ** -0.5).float()
    if mistake == 'zero_mean':
        mean[at[0], at[1]] = 0
    if mistake == 'neighbour':
        mean[at[0], at[1]] = mean[at[0], at[1] + 1]
        rstd[at[0], at[1]] = rstd[at[0], at[1] + 1]
    return mean, rstd


def staged_map(x, gamma, beta, film, mode, mean32, rstd32):
    """The staged element map in torch at the kernel's rounding points (gn_elem, nn_common.h): ga = f32(rstd gamma), gb = f32(beta - f32(mean ga)),
    y = f16(fma(x, ga, gb)) [-> f16(y f16(1 + f16(scale))) -> f16(y + f16(shift))] [-> f16(silu(y))] -> [N, H, W, C] f16."""
    C = x.shape[-1]
    m = mean32.repeat_interleave(C // 32, dim=1)[:, None, None, :]
    r = rstd32.repeat_interleave(C // 32, dim=1)[:, None, None, :]
    ga = r * gamma.float()
    gb = beta.float() - m * ga
    y = (x.double() * ga.double() + gb.double()).float().half()              # (one f32 rounding of the exact x ga + gb, then f16)
    if film is not None:
        t1 = (1.0 + film[:, :C].half().float()).half().float()[:, None, None, :]
        sh = film[:, C:].half().float()[:, None, None, :]
        y = (y.float() * t1).half()
        y = (y.float() + sh).half()
    if mode == 2:
        f = y.float()
        y = (f * torch.sigmoid(f)).half()
    return y


def group_ratio(got, ref, bound, n, g):
    """worst_ratio over the channels of group g of image n alone."""
    cg = got.shape[-1] // 32
    sl = slice(g * cg, (g + 1) * cg)
    return oc.worst_ratio(got[n, ..., sl], ref[n, ..., sl], bound[n, ..., sl])
