"""CPU-side checks of the C-ABI boundary: the library loads and exports every symbol include/pdhip.h declares,
argument validation returns error codes (no compute without a GPU), and the product refuses CPU tensors."""
import ctypes
import os
import re
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'pdhip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(pdhip_\w+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the UNet / DDNM entry points)
    L = _lib.lib()
    syms = declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/pdhip.h but not exported"
        assert s in _lib._SIGS, f"{s} has no ctypes signature in pointdreamer_amd/_lib.py"
    assert L.pdhip_version() >= 207
    assert L.pdhip_lab_build() == 0, "libpdhip.so carries a wrong-result PD_LAB_* timing switch: rebuild it without the flag"


def test_argument_validation_sets_error_message():
    from pointdreamer_amd import _lib
    L = _lib.lib()
    rc = L.pdhip_raster_mesh(None, 0, 0, None, 0, 0, None, None, None, None, None)
    assert rc == -1
    assert b'pdhip_raster_mesh' in L.pdhip_last_error()
    rc = L.pdhip_nearest_fill(None, None, 1, 3, 8, 8, 0, 0, 0, None, 0, 0, None, None)
    assert L.pdhip_nearest_fill_ws_ints(2, 256, 256) == 2 * 256 * 256 + 2 * 2 * 16 * 256      # near_row + first / last site per 16-row column segment
    assert rc == -1
    # the NBF path query and its hook are host-only: 0 bytes, 1 bits + pack16, 2 bits + ballot, 3 copy (include/pdhip.h)
    k = (ctypes.c_int32 * 2)(21, 11)
    assert [L.pdhip_nbf_path(2, 128, k, 2, m) for m in (0, 0x1, 0x10, 0x100)] == [1, 2, 0, 0] and L.pdhip_nbf_path(2, 100, k, 2, 0) == 0
    assert L.pdhip_nbf_path(2, 128, (ctypes.c_int32 * 1)(0), 1, 0) == 3
    assert L.pdhip_nbf_path(2, 128, (ctypes.c_int32 * 1)(20), 1, 0) == -1 and b'odd' in L.pdhip_last_error()
    assert L.pdhip_debug_set_nbf_path(1) == 0 and L.pdhip_nbf_path(2, 128, k, 2, 0) == 0 and L.pdhip_debug_set_nbf_path(0) == 1


def test_product_has_no_cpu_path():
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ours_utils as ou
    with pytest.raises(_lib.PdhipError):
        ou.get_point_pixels(torch.zeros((1, 4, 2)), 64)


def _non_docstring_strings(tree):
    """Every string constant of a module that is code (not a module / class / function docstring)."""
    import ast
    doc = set()
    for node in ast.walk(tree):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body and \
                isinstance(node.body[0], ast.Expr) and isinstance(node.body[0].value, ast.Constant) and isinstance(node.body[0].value.value, str):
            doc.add(id(node.body[0].value))
    return [n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and id(n) not in doc]


def test_product_never_imports_oracle():
    """The product package neither imports the oracle nor touches the reference checkout at run time: `/root/reference` may appear in
    docstrings and comments (file:line citations) only, never in a string the code can open, import or join."""
    import ast
    pkg = os.path.join(ROOT, 'pointdreamer_amd')
    seen = 0
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f"{f} imports the oracle"
                assert not re.search(r'import_module\(\s*[\'"]oracle', src), f"{f} imports the oracle dynamically"
                bad = [s for s in _non_docstring_strings(ast.parse(src)) if 'root/reference' in s or s.startswith('oracle.')]
                assert not bad, f"{f} carries a reference / oracle path in code: {bad[:2]}"
                seen += 1
    assert seen >= 15
    # the check itself must be able to fail: a code string with the path is caught, a docstring citation is not
    probe = ast.parse('def f():\n    "cites /root/reference/demo.py:1"\n    return open("/root/reference/x")\n')
    assert _non_docstring_strings(probe) == ["/root/reference/x"]


def test_ddnm_schedule_matches_reference_golden_on_host():
    """pdhip_ddnm_schedule is host-only arithmetic: alpha_bar table and (t, t_next) pairs bit-identical to the
    values the reference's Diffusion/compute_alpha produce (golden from tools/gen_golden_nn.py)."""
    import numpy as np
    from conftest import load_golden
    import pointdreamer_amd.ddnm_inpainting as di
    g = load_golden('ddnm_sampler.npz')
    at, an, t, tn, co = di.ddnm_schedule()
    assert np.array_equal(at, g['at']) and np.array_equal(an, g['at_next'])
    assert np.array_equal(t, g['t']) and np.array_equal(tn, g['t_next'])
    assert t[0] == 990 and tn[-1] == -1 and an[-1] == 1.0
    from oracle import ddnm as oddnm
    cos = oddnm.step_coefficients()
    for k in (0, 50, 99):
        ref = [cos[k][n].item() for n in ('sqrt_1m_at', 'sqrt_at', 'sqrt_at_next', 'sigma_t', 'c1', 'c2')]
        assert np.allclose(co[k], ref, rtol=2e-7, atol=0)


def test_halo_tile_conv_routing_table_on_host():
    """pdhip_conv_ht_plan (host-only): the automatic routing of the 256 x 64 halo-tile conv (csrc/nn_conv_ht.hip) over the
    UNet's 3x3 layer shapes -- 128^2 at batch 1 and at batch 2 from 512 input channels, 64^2 at batch 1-4 (two K-slabs at batch 1 from 512 input
    channels, which needs the split-K workspace), never 32^2, never beyond two rounds of workgroups."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401
    L = _lib.lib()
    WS = 16 * 384 * 128 * 128                                # the engine's split-K workspace (nn_unet.hip)

    def plan(N, HW, Cin, Cout, ws=WS):
        r, s = C.c_int(-1), C.c_int(-1)
        assert L.pdhip_conv_ht_plan(N, HW, HW, Cin, Cout, (Cout + 127) // 128 * 128, ws, C.byref(r), C.byref(s)) == 0
        return r.value, s.value

    assert plan(1, 128, 256, 256) == (1, 1) and plan(1, 128, 768, 256) == (1, 1) and plan(1, 128, 512, 512) == (1, 1)
    assert plan(2, 128, 256, 256)[0] == 0 and plan(2, 128, 512, 256) == (1, 1) and plan(2, 128, 512, 512)[0] == 0     # (1 024 tiles: the 512 x 128 tile's)
    assert plan(4, 128, 512, 256)[0] == 0
    assert plan(1, 64, 512, 512) == (1, 2) and plan(1, 64, 1024, 512) == (1, 2) and plan(1, 64, 768, 512) == (1, 2)      # (768 / 32 = 24 chunks: 12 per slab >= 8 -> two slabs)
    assert plan(1, 64, 256, 512) == (1, 1)                   # 4 chunks per slab would not pay for the combine
    assert plan(2, 64, 1024, 512) == (1, 1) and plan(4, 64, 512, 512) == (1, 1) and plan(8, 64, 512, 512)[0] == 0
    assert plan(1, 64, 1024, 512, ws=0) == (0, 1)            # no workspace: unsplit, and at half the chip the 1 024-channel layer is k_conv_sk's
    assert plan(1, 32, 512, 512)[0] == 0 and plan(1, 256, 256, 256)[0] == 0 and plan(1, 64, 48, 512)[0] == 0             # 32^2 / 256^2 / Cin % 32


# ---- pdhip_unet_route_table (host-only): the route of every conv of a UNet forward, planned without a device
ROUTE_SMALL = dict(image_size=32, num_channels=256, num_res_blocks=2, attention_resolutions="16,8", num_head_channels=64, channel_mult="1,2,4")


def _routes(N, **kw):
    """[(layer, HxW, Cin->Cout, kernel, detail, gn_chunks, set of folds)] of a batch-N forward (production config unless kw says otherwise)."""
    import pointdreamer_amd.ddnm_inpainting as di
    rows = []
    for line in di.unet_route_table(N, **kw):
        name, hw, ch, kernel, detail, gn, folds = line.split(' ')
        assert gn.startswith('gn=')
        rows.append((name, hw, ch, kernel, detail, int(gn[3:]), set() if folds == '-' else set(folds.split(','))))
    return rows


def test_unet_route_table_matches_the_committed_snapshot():
    """Production config (image 256, 256 channels, 2 ResBlocks per level, attention at 8 / 16 / 32, 64-channel heads, 6 outputs, the engine's split-K
    workspace) at batch 1, 2, 4, 8, 32: the table equals tests/golden/unet_route_table_256.txt, taken from the build whose kernel-launch sequence
    was compared, launch by launch, with the engine before the plan structs existed (profiles/route_plan_trace_check.txt)."""
    import __graft_entry__ as ge
    ge.build()
    import pointdreamer_amd.ddnm_inpainting as di
    got = ''.join(f"# N={N}\n" + '\n'.join(di.unet_route_table(N)) + '\n' for N in (1, 2, 4, 8, 32))
    want = open(os.path.join(ROOT, 'tests', 'golden', 'unet_route_table_256.txt')).read()
    assert got == want


@pytest.mark.parametrize("kw", [{}, ROUTE_SMALL], ids=["256", "32"])
def test_unet_route_table_is_consistent_at_every_batch(kw):
    """N = 1 ... 64: a row that takes res_up / in_up / apply names a kernel that can (res_up: rr, ht, sk or the unsplit halo kernel; in_up and apply:
    the halo kernel), and every conv whose input pass reads GroupNorm partials names producers, each a row that leaves some (gn > 0)."""
    import __graft_entry__ as ge
    ge.build()
    for N in range(1, 65):
        rows = _routes(N, **kw)
        gn = {r[0]: r[5] for r in rows}
        assert len(gn) == len(rows)                          # layer names are unique
        for name, _, _, kernel, detail, _, folds in rows:
            if 'res_up' in folds:
                assert kernel in ('rr', 'ht', 'sk') or (kernel == 'halo' and detail == 'splits=1'), (N, name, kernel, detail)
            if 'in_up' in folds or 'apply' in folds:
                assert kernel == 'halo', (N, name, kernel)
            if 'in_gn' in folds or 'skip' in folds:
                assert kernel in ('rr', 'sk') if 'skip' in folds else kernel == 'rr', (N, name, kernel)
            needs = [f for f in folds if f.startswith('parts<-')]
            assert needs or not ({'gn_skip', 'in_gn'} & folds), (N, name, folds)      # k_gn_skip and the in-staging GroupNorm read partials
            for f in needs:
                for producer in f[len('parts<-'):].split('+'):
                    assert gn.get(producer, 0) > 0, (N, name, producer)
        two = [r for r in rows if 'two_source' in r[6]]
        assert all(r[0].endswith('.skip_connection') for r in two)


def test_unet_route_table_follows_the_hooks():
    """up_phase 0 -> no phase rows, conv_rr mode 0 -> no rr rows, fold_skip 0 -> no +skip rows; every other row of the table stays as it was
    (apart from the rows of the blocks the hook changes), and the hooks are restored."""
    import __graft_entry__ as ge
    ge.build()
    from pointdreamer_amd import _lib
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401
    L = _lib.lib()
    for N in (1, 32):
        base = _routes(N)
        assert any(r[3] == 'phase' for r in base) and any('skip' in r[6] for r in base)
        assert any(r[3] == 'rr' for r in base) == (N == 1)
        hooks = [(lambda: L.pdhip_debug_set_up_phase(0), lambda old: L.pdhip_debug_set_up_phase(old), lambda r: r[3] == 'phase'),
                 (lambda: L.pdhip_debug_set_conv_rr(0, 0, 0), lambda old: L.pdhip_debug_set_conv_rr(old, 0, 0), lambda r: r[3] == 'rr'),
                 (lambda: L.pdhip_debug_set_fold_skip(0), lambda old: L.pdhip_debug_set_fold_skip(old), lambda r: 'skip' in r[6])]
        for flip, restore, hit in hooks:
            old = flip()
            try:
                off = _routes(N)
            finally:
                restore(old)
            assert not any(hit(r) for r in off)
            block = lambda r: re.match(r'(input_blocks|output_blocks)\.\d+\.\d+|middle_block\.\d+', r[0]).group(0)
            changed = {block(r) for r in base if hit(r)}     # the blocks whose rows the hook touches
            assert [r for r in off if block(r) not in changed] == [r for r in base if block(r) not in changed]
            assert _routes(N) == base                        # restored


def test_unet_route_table_under_every_hook_matches_the_recorded_digests():
    """Production config at batch 1, 2, 8, 32 with every routing / fold hook flipped alone to each of its documented non-default values
    (nn_hooks_common.ROUTE_SETTINGS): row count and SHA-256 of each table equal tests/golden/unet_route_table_hooks.txt, recorded from the build
    before the hooks became one Tuning struct handed to the planners (tools/gen_route_table_hooks.py writes the file and prints a full table).
    Every hook is restored in a finally (nn_hooks_common.hook); the last step is the default table again."""
    import __graft_entry__ as ge
    ge.build()
    import nn_hooks_common as nh
    want = {}
    for line in open(os.path.join(ROOT, 'tests', 'golden', 'unet_route_table_hooks.txt')):
        label, n, rows, sha = line.split()
        want[(label, int(n[2:]))] = (int(rows[5:]), sha[7:])
    settings = [('default', None, ())] + nh.ROUTE_SETTINGS
    assert set(want) == {(label, N) for label, _, _ in settings for N in nh.ROUTE_BATCHES} and len(settings) == 29
    default = {N: nh.route_table_lines('default', None, (), N) for N in nh.ROUTE_BATCHES}
    for label, setter, args in settings:
        for N in nh.ROUTE_BATCHES:
            assert nh.route_table_digest(nh.route_table_lines(label, setter, args, N)) == want[(label, N)], (label, N)
    for N in nh.ROUTE_BATCHES:
        assert nh.route_table_lines('default', None, (), N) == default[N], N      # every hook is back at its default
