"""The UNet engine's tuning hooks (the pdhip_debug_set_* entry points over csrc/nn_common.h's Tuning) for the tests: one context manager that sets
a hook and puts the shipped default back on the way out, whatever the body does, and the list of settings tests/golden/unet_route_table_hooks.txt
records (tools/gen_route_table_hooks.py writes that file).  A hook left set would route every later test of the pytest process differently."""
import contextlib

# setter (without the pdhip_debug_set_ prefix) -> the arguments that put the shipped defaults back (Tuning's initialisers).
# conv_splitk's pointer argument is the stand-alone conv entry's workspace: state, not tuning; NULL is what a fresh process has.
DEFAULTS = {
    'conv_tile': (0,), 'conv_bk': (0,), 'conv_stages': (0,), 'conv_splitk': (None, 0, 0), 'conv_halo_strips': (0,),
    'conv_sk': (1, 0, 0), 'conv_sk_stages': (0,), 'conv_sk_kgroups': (0,), 'conv_sk_order': (0,),
    'conv_rr': (1, 0, 0), 'conv_ht': (1, 0),
    'fuse_gn': (0,), 'fold_resample': (1,), 'fold_skip': (1,), 'rr_gn': (0,), 'fold_finalize': (8,), 'fold_finalize_chunks': (16,),
    'fuse_skip': (1, 1), 'up_phase': (1,),
    'attn': (0, 0, 0), 'gn_iters': (0,), 'gn_skip_variant': (1,),
}


def _lib():
    from pointdreamer_amd import _lib as lib_mod
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the hooks' signatures)
    return lib_mod.lib()


@contextlib.contextmanager
def hook(name, *args):
    """with hook('conv_sk', 2, 4, 0): ...  -- pdhip_debug_set_conv_sk(2, 4, 0) for the body, the default afterwards."""
    setter = getattr(_lib(), 'pdhip_debug_set_' + name)
    default = DEFAULTS[name]
    assert len(args) == len(default), (name, args)
    setter(*args)
    try:
        yield
    finally:
        setter(*default)


# every routing / fold hook alone at each of its documented non-default values: (label, setter, arguments)
ROUTE_SETTINGS = (
    [(f'conv_tile={v}', 'conv_tile', (v,)) for v in (2, 4, 8, 32)] +
    [('conv_bk=32', 'conv_bk', (32,)), ('conv_stages=3', 'conv_stages', (3,)), ('conv_splits=4', 'conv_splitk', (None, 0, 4)),
     ('conv_halo_strips=1', 'conv_halo_strips', (1,))] +
    [('conv_sk=%d,%d,%d' % a, 'conv_sk', a) for a in ((0, 0, 0), (2, 0, 0), (2, 3, 2))] +
    [('conv_rr=%d,%d,%d' % a, 'conv_rr', a) for a in ((0, 0, 0), (2, 0, 0), (2, 5, 2))] +
    [('conv_ht=%d,%d' % a, 'conv_ht', a) for a in ((0, 0), (2, 0), (2, 2))] +
    [('fuse_gn=1', 'fuse_gn', (1,)), ('fold_resample=0', 'fold_resample', (0,)), ('fold_skip=0', 'fold_skip', (0,))] +
    [(f'rr_gn={v}', 'rr_gn', (v,)) for v in (8, 16, 32)] +
    [('fold_finalize=0', 'fold_finalize', (0,))] +
    [(f'fuse_skip={v}', 'fuse_skip', (v, 1)) for v in (0, 2)] +
    [(f'up_phase={v}', 'up_phase', (v,)) for v in (0, 2)])
ROUTE_BATCHES = (1, 2, 8, 32)


def route_table_lines(label, setter, args, N):
    """The production config's route table at batch N with one hook set (label 'default': none)."""
    import pointdreamer_amd.ddnm_inpainting as di
    if label == 'default':
        return di.unet_route_table(N)
    with hook(setter, *args):
        return di.unet_route_table(N)


def route_table_digest(lines):
    import hashlib
    return len(lines), hashlib.sha256(('\n'.join(lines) + '\n').encode()).hexdigest()
