"""demo.py-compatible driver for the texturing path: same CLI (`--config`, `--pc_file` file-or-directory),
same YAML keys (configs/*.yaml of the reference) and the same output tree as /root/reference/demo.py:311-497:

  <output_path>/<ply stem>_<config stem>/config.yaml, input_pc.ply,
      models/model_normalized.{obj,mtl,png}, others/{k}_{sparse,mask0,mask2,inpainted}.png, others/atlas_wo_background.png
      and, only with the opt-in key `render_views` (6 or 20; `render_res`, default 512): rendered_imgs/albedo_%03d.png

A cloud above 30 000 points is refused as in the reference (demo.py:371-374) unless the opt-in key `subsample: fps` is set: then it is subsampled on
the device to `subsample_num` points (default 30 000) by farthest-point sampling, `subsample_colors: mean` averaging the colours each sample stands
for; input_pc.ply is the subsample, and `geo_from: 'SPR'` still reconstructs from the full cloud.

With the opt-in key `remove_outliers: statistical` (`outlier_neighbors`, default 20; `outlier_std_ratio`, default 2.0) the raw cloud first loses the
points whose mean distance to their nearest neighbours lies above mean + ratio * std of that quantity (outliers.py): the point limit, the box
normalisation, a supplied mesh's normalisation, SPR and `subsample` see only the kept points; the removed ones go to others/removed_outliers.ply.

With the opt-in keys `spr_components: largest` / `spr_min_component_share` the mesh reconstructed under `geo_from: 'SPR'` loses its small floating
pieces on the device (mesh_components.py) before it is decimated, cached and textured; elsewhere the keys have no effect.

With the opt-in key `spr_smooth: <steps>` (`spr_smooth_lambda`, default 0.5; `spr_smooth_mu`, default -0.53: MeshLab's Taubin pair) the vertices of
that mesh are smoothed on the device (mesh_smooth.py) after the components filter and before the decimation; faces and colours stay as they are.

Geometry: the reference's drop-in hooks -- `<pc>_untextured_mesh.obj` next to the PLY (demo.py:391-399), the cached
`geo/<name>_untextured/models/model_normalized.obj` (demo.py:401-406) and the cached `geo/xatlas_<res>.pth` dict (demo.py:428-448)
-- and, with `geo_from: 'SPR'`, a mesh reconstructed from the cloud on the device (spr.recon_one_shape_SPR; POCO stays out of
scope).  A mesh without `vt` records is unwrapped on the device (extract_texture_map.xatlas_uvmap_w_face_id, this
build's own chart layout) and the dict cached; if no mesh is supplied and `geo_from` is not 'SPR' it falls back to the build's stand-in UV sphere fitted to
the cloud (clearly logged), so that the texturing path can be exercised end to end.

  python -m pointdreamer_amd.demo --config configs/nearest.yaml --pc_file dataset/demo_data/clock.ply
"""
import argparse
import datetime
import logging
import os
import shutil
import time

import numpy as np
import PIL.Image
import torch
import yaml

from . import io_utils, pipeline, synthetic
from .camera_utils import create_cameras

SUPPORTED_KEYS = ('texture_gen_method', 'camera_distribution', 'cam_res', 'view_num', 'res', 'point_size', 'edge_point_size',
                  'point_validation_by_o3d', 'hidden_point_removal_radius', 'refine_point_validation_by_remove_abnormal_depth',
                  'crop_img', 'crop_padding', 'mask_ratio_thresh', 'edge_dilate_kernels', 'optimize_from',
                  'xatlas_texture_res', 'complete_unseen_by', 'output_path')
# keys of this build's own stages in front of the texturing path (geo_from: 'SPR'): validated like the others, not pipeline arguments
GEOMETRY_KEYS = ('spr_depth', 'spr_knn', 'spr_faces')
# opt-in stage behind the texturing path: render_views (6 or 20 'self_defined' views) writes <out>/rendered_imgs/albedo_%03d.png at
# render_res (default 512); without render_views nothing is rendered and the output tree is unchanged
RENDER_KEYS = ('render_views', 'render_res')
# opt-in stage in front of everything: subsample: 'fps' takes a cloud above SUBSAMPLE_LIMIT points down to subsample_num (default and at most the
# limit) by farthest-point sampling on the device (subsample.py); subsample_colors: 'point' (default) keeps the samples' own colours, 'mean' gives each
# sample the mean colour of the points it stands for.  Without `subsample` such a cloud is refused as in the reference
SUBSAMPLE_KEYS = ('subsample', 'subsample_num', 'subsample_colors')
SUBSAMPLE_LIMIT = 30000
# opt-in stage in front of that: remove_outliers: 'statistical' drops the points whose mean distance to their outlier_neighbors (default 20) nearest
# neighbours lies above mean + outlier_std_ratio (default 2.0) * std of that quantity (outliers.py), on the raw coordinates, before the point limit
# and the box normalisation; the removed points go to others/removed_outliers.ply.  Without the key nothing is filtered
OUTLIER_KEYS = ('remove_outliers', 'outlier_neighbors', 'outlier_std_ratio')
# opt-in stage behind the SPR reconstruction (geo_from: 'SPR' only, before spr_faces' decimation): spr_components: 'largest' keeps the component of the
# reconstructed mesh with the most faces ('all', the default when absent: every component, as before); spr_min_component_share (a float in (0, 1])
# keeps the components with at least that share of the largest one's face count (mesh_components.py).  The cached geometry OBJ is the filtered mesh
COMPONENT_KEYS = ('spr_components', 'spr_min_component_share')
# opt-in stage behind that one (geo_from: 'SPR' only, still before spr_faces' decimation): spr_smooth: the number of Taubin steps (mesh_smooth.py) that
# smooth the vertices of the reconstructed mesh, with spr_smooth_lambda (default 0.5) and spr_smooth_mu (default -0.53; 0: the plain Laplacian).
# The cached geometry OBJ is the smoothed mesh; without spr_smooth nothing is smoothed
SMOOTH_KEYS = ('spr_smooth', 'spr_smooth_lambda', 'spr_smooth_mu')
# opt-in stage in front of everything a SUPPLIED `<pc>_untextured_mesh.obj` goes through (not the SPR mesh, which marching cubes welds): mesh_clean:
# 'weld' merges its close vertices and drops degenerate faces, duplicate faces and unreferenced vertices (mesh_clean.py) after loading and before
# the normalisation; mesh_weld_tolerance (default 0: exactly equal coordinates) is the welding distance as a share of the mesh's box diagonal, in
# [0, 0.1], as MeshLab's percentage is.  The atlas cache of such a run is xatlas_<res>_weld.pth: it never shares one with a run without the key
CLEAN_KEYS = ('mesh_clean', 'mesh_weld_tolerance')
# opt-in stage behind that one, on a SUPPLIED mesh too (after the cleaning if that ran, before the normalisation): mesh_orient: 'coherent' makes the
# faces of every patch agree and turns closed patches outward (mesh_orient.py); mesh_orient_open: 'majority' (default: an open patch keeps the winding of
# most of its faces) or 'volume' (open patches follow the closed patches' rule).  The `ft` rows of flipped faces get the same (1, 2) swap, and the atlas
# cache name gains _orient
ORIENT_KEYS = ('mesh_orient', 'mesh_orient_open')


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def get_logger(path):
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    logger = logging.getLogger('pointdreamer_amd')
    logger.setLevel(logging.INFO)
    if not logger.handlers:
        fmt = logging.Formatter('%(asctime)s %(levelname)s %(message)s')
        for h in (logging.FileHandler(path), logging.StreamHandler()):
            h.setFormatter(fmt)
            logger.addHandler(h)
    return logger


# keys of the reference's configs/*.yaml that steer stages UPSTREAM or outside of the texturing path (dataset bookkeeping, POCO / SPR
# geometry, evaluation): accepted verbatim and ignored, so that the reference's five YAML files load unchanged
UPSTREAM_KEYS = ('exp_name', 'exist_root_path', 'dataset_name', 'cls_id', 'input_pc_generate_method', 'demo', 'geo_root', 'geo_from',
                 'load_exist_dense_img_path', 'use_GT_geo_watertight', 'use_GT_multi_view_img', 'noise_stddev', 'coords_scale',
                 'input_type', 'input_already_noisy', 'save_dir', 'render_after_inference', 'save_input_pc', 'project2mesh',
                 'refine_res', 'smooth_mesh', 'sample_num')
DEFAULTS = dict(camera_distribution='fibonacci_sphere', cam_res=512, view_num=8, res=256, point_size=1, edge_point_size=1,
                point_validation_by_o3d=True, hidden_point_removal_radius=100, refine_point_validation_by_remove_abnormal_depth=False,
                crop_img=True, crop_padding=0.05, mask_ratio_thresh=0.82, edge_dilate_kernels=[21], optimize_from='ours',
                xatlas_texture_res=1024, complete_unseen_by='neighbor', output_path='output')


def load_config(cfg_file, overrides=None):
    """demo.py:313-314 (`Munch.fromDict(yaml.safe_load(...))`): the reference's YAML files load as they are.  Keys the path reads
    are validated, upstream keys are kept but unused, an unknown key is an error (a typo must not silently fall back)."""
    cfg = Cfg(yaml.safe_load(open(cfg_file)))
    cfg.update(overrides or {})
    unknown = [k for k in cfg if k not in SUPPORTED_KEYS and k not in UPSTREAM_KEYS and k not in GEOMETRY_KEYS and k not in RENDER_KEYS
               and k not in SUBSAMPLE_KEYS and k not in OUTLIER_KEYS and k not in COMPONENT_KEYS and k not in SMOOTH_KEYS and k not in CLEAN_KEYS
               and k not in ORIENT_KEYS]
    if unknown:
        raise KeyError(f"{cfg_file}: unknown config keys {unknown}")
    if 'texture_gen_method' not in cfg:
        raise KeyError(f"{cfg_file}: texture_gen_method is required")
    for k, v in DEFAULTS.items():
        cfg.setdefault(k, v)
    # camera_utils.py:116-245: 'blender' / 'exact_blender' always place 20 cameras, 'self_defined' knows 6 or 20 -- the per-view
    # arrays of the path are sized by view_num, so a mismatch is an error here instead of an index error later
    if cfg.camera_distribution in ('blender', 'exact_blender') and cfg.view_num != 20:
        raise ValueError(f"camera_distribution={cfg.camera_distribution!r} places 20 cameras: set view_num: 20 (got {cfg.view_num})")
    from . import spr
    if 'spr_depth' in cfg and cfg.spr_depth not in spr.DEPTHS:
        raise ValueError(f"spr_depth={cfg.spr_depth!r}: the dense grid of the SPR geometry supports {spr.DEPTHS} (2^depth cells per axis)")
    if 'spr_knn' in cfg and not (isinstance(cfg.spr_knn, int) and 3 <= cfg.spr_knn <= 32):
        raise ValueError(f"spr_knn={cfg.spr_knn!r}: the normals of the SPR geometry take 3 .. 32 neighbours")
    if 'spr_faces' in cfg and not (isinstance(cfg.spr_faces, int) and not isinstance(cfg.spr_faces, bool) and cfg.spr_faces >= 4):
        raise ValueError(f"spr_faces={cfg.spr_faces!r}: the face count the SPR geometry is decimated to is an integer >= 4")
    if 'render_views' in cfg and cfg.render_views not in (6, 20):
        raise ValueError(f"render_views={cfg.render_views!r}: the 'self_defined' evaluation cameras come as 6 or 20 views")
    if 'render_res' in cfg and not (isinstance(cfg.render_res, int) and not isinstance(cfg.render_res, bool) and 1 <= cfg.render_res <= 16384):
        raise ValueError(f"render_res={cfg.render_res!r}: the side of the rendered views is an integer in 1 .. 16384")
    if 'subsample' in cfg and cfg.subsample not in ('fps',):
        raise ValueError(f"subsample={cfg.subsample!r}: the subsampler of clouds above {SUBSAMPLE_LIMIT} points is 'fps' (farthest point)")
    if 'subsample_num' in cfg and not (isinstance(cfg.subsample_num, int) and not isinstance(cfg.subsample_num, bool)
                                       and 1 <= cfg.subsample_num <= SUBSAMPLE_LIMIT):
        raise ValueError(f"subsample_num={cfg.subsample_num!r}: the size of the subsample is an integer in 1 .. {SUBSAMPLE_LIMIT}")
    if 'subsample_colors' in cfg and cfg.subsample_colors not in ('point', 'mean'):
        raise ValueError(f"subsample_colors={cfg.subsample_colors!r}: 'point' (the samples' own colours) or 'mean' (of the points each stands for)")
    if 'remove_outliers' in cfg and cfg.remove_outliers not in ('statistical',):
        raise ValueError(f"remove_outliers={cfg.remove_outliers!r}: the outlier filter is 'statistical' (mean k-NN distance against mean + ratio * std)")
    if 'outlier_neighbors' in cfg and not (isinstance(cfg.outlier_neighbors, int) and not isinstance(cfg.outlier_neighbors, bool)
                                           and 1 <= cfg.outlier_neighbors <= 63):
        raise ValueError(f"outlier_neighbors={cfg.outlier_neighbors!r}: the neighbours of the outlier filter are an integer in 1 .. 63")
    if 'outlier_std_ratio' in cfg and not (isinstance(cfg.outlier_std_ratio, (int, float)) and not isinstance(cfg.outlier_std_ratio, bool)
                                           and 0.0 <= cfg.outlier_std_ratio < float('inf')):
        raise ValueError(f"outlier_std_ratio={cfg.outlier_std_ratio!r}: the ratio of the outlier filter is a finite number >= 0")
    if 'spr_components' in cfg and cfg.spr_components not in ('all', 'largest'):
        raise ValueError(f"spr_components={cfg.spr_components!r}: the components kept of the SPR geometry are 'all' or 'largest' (the one with the most faces)")
    if 'spr_min_component_share' in cfg and not (isinstance(cfg.spr_min_component_share, (int, float))
                                                 and not isinstance(cfg.spr_min_component_share, bool) and 0.0 < cfg.spr_min_component_share <= 1.0):
        raise ValueError(f"spr_min_component_share={cfg.spr_min_component_share!r}: the share of the largest component's face count that a component "
                         "of the SPR geometry needs is a number in (0, 1]")
    if any(k in cfg for k in SMOOTH_KEYS):
        from . import mesh_smooth
        if 'spr_smooth' not in cfg:
            raise ValueError("spr_smooth_lambda / spr_smooth_mu steer the smoothing that spr_smooth: <steps> asks for: spr_smooth is missing")
        try:
            mesh_smooth.check_params(cfg.spr_smooth, cfg.get('spr_smooth_lambda', mesh_smooth.DEFAULT_LAMBDA),
                                     cfg.get('spr_smooth_mu', mesh_smooth.DEFAULT_MU))
        except ValueError as e:
            raise ValueError(f"spr_smooth={cfg.spr_smooth!r}, spr_smooth_lambda={cfg.get('spr_smooth_lambda')!r}, "
                             f"spr_smooth_mu={cfg.get('spr_smooth_mu')!r}: {e}") from None
    if 'mesh_clean' in cfg and cfg.mesh_clean not in ('weld',):
        raise ValueError(f"mesh_clean={cfg.mesh_clean!r}: the cleaning of a supplied mesh is 'weld' (merge close vertices, drop degenerate and "
                         "duplicate faces and unreferenced vertices)")
    if 'mesh_weld_tolerance' in cfg:
        if 'mesh_clean' not in cfg:
            raise ValueError("mesh_weld_tolerance steers the welding that mesh_clean: weld asks for: mesh_clean is missing")
        t = cfg.mesh_weld_tolerance
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0.0 <= t <= 0.1:
            raise ValueError(f"mesh_weld_tolerance={t!r}: the welding distance is a share of the mesh's box diagonal in [0, 0.1]")
    if 'mesh_orient' in cfg and cfg.mesh_orient not in ('coherent',):
        raise ValueError(f"mesh_orient={cfg.mesh_orient!r}: the orientation of a supplied mesh is 'coherent' (the faces of every patch agree, closed "
                         "patches face outward)")
    if 'mesh_orient_open' in cfg:
        if 'mesh_orient' not in cfg:
            raise ValueError("mesh_orient_open steers the orientation that mesh_orient: coherent asks for: mesh_orient is missing")
        if cfg.mesh_orient_open not in ('majority', 'volume'):
            raise ValueError(f"mesh_orient_open={cfg.mesh_orient_open!r}: open patches are oriented by 'majority' or by 'volume'")
    if cfg.optimize_from == 'None':                      # YAML `None` is the string 'None' (demo.py:213 treats both alike)
        cfg['optimize_from'] = None
    return cfg


def prepare(cfg_file, device, ckpt_path=None, allow_random_weights=False, overrides=None, batch_shapes=1):
    """demo.py:311-356 without the POCO network."""
    cfg = load_config(cfg_file, overrides)
    rank = int(os.environ.get('RANK', 0))
    stamp = datetime.datetime.now().strftime("%Y.%m.%d.%H.%M.%S") + (f'_rank{rank}' if int(os.environ.get('WORLD_SIZE', 1)) > 1 else '')
    logger = get_logger(os.path.join(cfg.output_path, f'{stamp}_log.log'))
    inpainter = None
    if cfg.texture_gen_method == 'DDNM_inpaint':
        logger.info('Loading inpainter...')
        from .ddnm_inpainting import Inpainter, DEFAULT_CKPT
        inpainter = Inpainter(device, ckpt_path=ckpt_path or DEFAULT_CKPT, allow_random_weights=allow_random_weights,
                              max_batch=cfg.view_num * max(1, int(batch_shapes)))
        logger.info('inpainter loaded')
    cams, base_dirs, eye_positions, up_dirs = create_cameras(num_views=cfg.view_num, distribution=cfg.camera_distribution,
                                                             distance=1.6, res=cfg.cam_res, device=device)
    camera_info = dict(cams=cams, base_dirs=base_dirs, eye_positions=eye_positions, up_dirs=up_dirs)
    return cfg, inpainter, camera_info, logger


_STANDIN = {}


def standin_geometry(xyz, atlas_res, device, logger):
    """No mesh next to the PLY and no POCO here: UV sphere (radius 0.5 = the normalised cloud's half extent) + analytic atlas.
    The same for every cloud, so a directory run builds it once per (atlas_res, device)."""
    logger.warning('no <pc>_untextured_mesh.obj supplied: using the stand-in UV sphere geometry (POCO/SPR are upstream)')
    key = (int(atlas_res), str(device))
    if key not in _STANDIN:
        _STANDIN[key] = _standin_geometry(atlas_res, device)
    v, f, d = _STANDIN[key]
    return v.clone(), f.clone(), {k: t.clone() for k, t in d.items()}


def _standin_geometry(atlas_res, device):
    verts, faces, lut = synthetic.uv_sphere(50, 100)
    gb_pos, mask, fid = synthetic.latlong_atlas(atlas_res, 50, 100, lut=lut)
    # per-corner UVs of the lat-long parametrisation (one vt per face corner, like xatlas' unshared output)
    v = verts.astype(np.float64)
    lat = np.arccos(np.clip(v[:, 1] / 0.5, -1, 1)) / np.pi
    lon = (np.arctan2(v[:, 2], v[:, 0]) % (2 * np.pi)) / (2 * np.pi)
    corner_uv = np.stack([lon[faces], lat[faces]], -1)                          # [F,3,2]
    wrap = (corner_uv[..., 0].max(1) - corner_uv[..., 0].min(1)) > 0.5           # faces crossing the seam
    cu = corner_uv[..., 0]
    cu[wrap] = np.where(cu[wrap] < 0.5, cu[wrap] + 1.0, cu[wrap])
    span, g = atlas_res - 4, 2
    uvs = np.stack([(np.clip(cu, 0, 1) * span + g) / atlas_res, (corner_uv[..., 1] * span + g) / atlas_res], -1).reshape(-1, 2)
    tex_idx = np.arange(faces.shape[0] * 3, dtype=np.int64).reshape(-1, 3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return T(verts), T(faces), dict(uvs=T(uvs.astype(np.float32)), mesh_tex_idx=T(tex_idx), gb_pos=T(gb_pos), mask=T(mask),
                                    per_atlas_pixel_face_id=T(fid))


def save_textured_mesh(vertices, uvs, faces, mesh_tex_idx, atlas_img, mask, output_root_path):
    """demo.py:264-307."""
    io_utils.savemeshtes2(vertices.cpu().numpy(), uvs.cpu().numpy(), faces.cpu().numpy(), mesh_tex_idx.cpu().numpy(),
                          os.path.join(output_root_path, 'models', 'model_normalized.obj'))
    # atlas [A,A,3] -> flipped vertically, uint8(clip(x*255)), PNG (device conversion + native encoder)
    io_utils.save_CHW_RGB_img(atlas_img.flip(0).permute(2, 0, 1), os.path.join(output_root_path, 'models', 'model_normalized.png'))
    # others/atlas_wo_background.png: the atlas with the chart mask as alpha (demo.py:296-303)
    rgba = torch.cat([atlas_img.float(), mask[0].to(atlas_img.device).float()], dim=-1)
    io_utils.save_CHW_RGBA_img(rgba.flip(0).permute(2, 0, 1), os.path.join(output_root_path, 'others', 'atlas_wo_background.png'))


def render_result(cfg, vertices, uvs, faces, mesh_tex_idx, atlas_img, output_root_path, device, logger):
    """The opt-in `render_views` stage: the in-memory result from the 'self_defined' evaluation cameras (camera_utils.py:165-201, as
    render_textured_meshes_shapenet2 places them) -> <out>/rendered_imgs/albedo_%03d.png, RGBA.  Nothing without the key."""
    if 'render_views' not in cfg:
        return None
    from .camera_utils import render_textured_mesh2
    start = time.time()
    cams, _, _, _ = create_cameras(num_views=cfg.render_views, distribution='self_defined', distance=1.6,
                                   res=cfg.get('render_res', 512), device=device)
    save_path = os.path.join(output_root_path, 'rendered_imgs')
    render_textured_mesh2(vertices, faces, uvs, mesh_tex_idx, atlas_img, cams, save_path=save_path, save=True)
    logger.info(f'rendered {cfg.render_views} views at {cfg.get("render_res", 512)}^2 -> {save_path} ({time.time() - start} s)')
    return save_path


def _remove_outliers(cfg, xyz, rgb, out, device, logger):
    """The opt-in `remove_outliers` stage on the raw cloud as read from the PLY: (xyz, rgb) of the kept points, in the file's order; the removed
    points -> <out>/others/removed_outliers.ply."""
    from . import outliers
    start = time.time()
    xyz, rgb = np.asarray(xyz, np.float32), np.asarray(rgb)
    k, ratio = cfg.get('outlier_neighbors', 20), cfg.get('outlier_std_ratio', 2.0)
    keep, st = outliers.statistical_outlier_mask(torch.from_numpy(np.ascontiguousarray(xyz)).to(device), nb_neighbors=k, std_ratio=ratio,
                                                 return_stats=True)
    keep = keep.cpu().numpy()
    # (the writer stores uint8(c * 255), truncating: the half keeps every byte of the file's colours)
    io_utils.save_colored_pc_ply(xyz[~keep], (np.asarray(rgb[~keep], np.float32) + 0.5) / 255.0, os.path.join(out, 'others', 'removed_outliers.ply'))
    logger.info(f'statistical outlier removal ({k} neighbours, ratio {ratio}): kept {st["kept"]}, removed {st["removed"]} of {len(xyz)} points '
                f'(mean {st["mean"]:.6g}, std {st["std"]:.6g}, threshold {st["threshold"]:.6g}; {time.time() - start} s)')
    return xyz[keep], rgb[keep]


def _component_rules(cfg):
    """The opt-in COMPONENT_KEYS as recon_one_shape_SPR's keyword: nothing without them (or with spr_components: 'all' alone), so that nothing new runs."""
    rules = {}
    if cfg.get('spr_components', 'all') == 'largest':
        rules['keep'] = 'largest'
    if 'spr_min_component_share' in cfg:
        rules['min_face_share'] = float(cfg.spr_min_component_share)
    return dict(keep_components=rules) if rules else {}


def _smooth_rules(cfg):
    """The opt-in SMOOTH_KEYS as recon_one_shape_SPR's keyword: nothing without spr_smooth, so that nothing new runs."""
    if 'spr_smooth' not in cfg:
        return {}
    from . import mesh_smooth
    return dict(smooth=dict(steps=int(cfg.spr_smooth), lam=float(cfg.get('spr_smooth_lambda', mesh_smooth.DEFAULT_LAMBDA)),
                            mu=float(cfg.get('spr_smooth_mu', mesh_smooth.DEFAULT_MU))))


def _clean_supplied(cfg, vertices, faces, ft, logger):
    """The opt-in CLEAN_KEYS on a supplied mesh: (vertices, faces, ft) welded and cleaned; the `ft` rows (numpy, or None) follow the kept faces."""
    from . import mesh_clean
    box = (vertices.max(0)[0] - vertices.min(0)[0]).double()
    tol = float(cfg.get('mesh_weld_tolerance', 0.0)) * float((box * box).sum().sqrt())
    v, f, fidx, c = mesh_clean.clean_mesh(vertices, faces, tolerance=tol, return_face_index=True, return_counts=True)
    rep = mesh_clean.mesh_report(v, f)
    logger.info(f'mesh_clean: weld at tolerance {tol:.6g}: vertices {c["vertices_before"]} -> {c["vertices_after"]} ({c["merged"]} merged, '
                f'{c["unreferenced"]} unreferenced), faces {c["faces_before"]} -> {c["faces_after"]} ({c["degenerate"]} degenerate, {c["duplicate"]} '
                f'duplicate); after cleaning: {rep["boundary_edges"]} boundary edges, {rep["nonmanifold_pairs"]} non-manifold edges, '
                f'{rep["components"]} components')
    if ft is not None:
        ft = np.ascontiguousarray(ft[fidx.cpu().numpy()])
    return v, f, ft


def _orient_supplied(cfg, vertices, faces, ft, logger):
    """The opt-in ORIENT_KEYS on a supplied mesh: faces coherently oriented; the `ft` rows (numpy, or None) of flipped faces get the same swap."""
    from . import mesh_orient
    rule = cfg.get('mesh_orient_open', 'majority')
    f, flip, c = mesh_orient.orient_faces(vertices, faces, open_patches=rule, return_flip=True, return_counts=True)
    logger.info(f'mesh_orient: coherent (open patches by {rule}): {c["patches"]} patches, {c["flipped"]} of {len(f)} faces flipped, '
                f'{c["nonorientable_patches"]} non-orientable patches, {c["incoherent_edges"]} incoherent edges before')
    if ft is not None:
        m = flip.cpu().numpy().astype(bool)
        ft = np.ascontiguousarray(ft).copy()
        ft[m] = ft[m][:, [0, 2, 1]]
    return f, ft


def _load_shape(cfg, pc_file, name, device, logger):
    """demo.py:359-452: cloud, mesh and atlas of one shape, normalised as the reference does."""
    out = os.path.join(cfg.output_path, name)
    for d in ('geo', 'models', 'others'):
        os.makedirs(os.path.join(out, d), exist_ok=True)
    xyz, rgb = io_utils.read_ply_xyzrgb(pc_file)
    if 'remove_outliers' in cfg:
        xyz, rgb = _remove_outliers(cfg, xyz, rgb, out, device, logger)
    if len(xyz) > 30000 and 'subsample' not in cfg:
        print(f"Point number > 30000! ({len(xyz)} points)({pc_file}) \n Please try uniformly subsampling the input point cloud first")
        raise NotImplementedError
    xyz = torch.tensor(np.asarray(xyz, np.float32)).to(device)
    rgb = torch.tensor(np.asarray(rgb)).float().to(device) / 255.0
    vmin, vmax = xyz.min(0)[0], xyz.max(0)[0]
    xyz -= (vmax + vmin) / 2.
    xyz /= (vmax - vmin).max()
    # above the limit (only with `subsample`): the cloud is normalised by its FULL box, so that a supplied mesh still lines up; the SPR geometry
    # below reconstructs from the full cloud, the texturing path gets the subsample
    full = (xyz, rgb) if len(xyz) > SUBSAMPLE_LIMIT else None
    if full is not None:
        from . import subsample
        start = time.time()
        xyz, rgb, _, min_d2 = subsample.subsample_cloud(full[0], full[1], num=cfg.get('subsample_num', SUBSAMPLE_LIMIT),
                                                        colors_from=cfg.get('subsample_colors', 'point'), return_min_d2=True)
        radius = float(min_d2[-1].sqrt()) if len(xyz) > 1 else float('inf')
        logger.info(f'subsampled {len(full[0])} -> {len(xyz)} points by farthest-point sampling (covering radius {radius:.6g}, colours: '
                    f'{cfg.get("subsample_colors", "point")}; {time.time() - start} s)')
    io_utils.save_colored_pc_ply(xyz.cpu().numpy(), rgb.cpu().numpy(), os.path.join(out, 'input_pc.ply'))
    geo_path = pc_file.replace('.ply', '_untextured_mesh.obj')
    weld = 'mesh_clean' in cfg and os.path.exists(geo_path)       # (the key touches a supplied mesh only)
    orient = 'mesh_orient' in cfg and os.path.exists(geo_path)   # (likewise)
    xatlas_file = os.path.join(out, 'geo', f'xatlas_{cfg.xatlas_texture_res}{"_weld" if weld else ""}{"_orient" if orient else ""}.pth')
    cached_geo = os.path.join(out, 'geo', f'{name}_untextured', 'models', 'model_normalized.obj')
    if not os.path.exists(geo_path) and not os.path.exists(cached_geo) and cfg.get('geo_from') == 'SPR':
        # baselines/spr.py:recon_one_shape_SPR on the normalised cloud (demo.py:411-416), on the device; the mesh goes to the
        # reference's cache path and is read back from it, so that this run and a resumed one texture the same float32 values
        from . import spr
        logger.info('Generating geometry by SPR...')
        start = time.time()
        depth = cfg.get('spr_depth', spr.DEFAULT_DEPTH)
        geo_xyz, geo_rgb = full if full is not None else (xyz, rgb)
        rv, rf, _, rc = spr.recon_one_shape_SPR(geo_xyz, geo_rgb, depth=depth, knn=cfg.get('spr_knn', spr.DEFAULT_KNN), save_path=cached_geo,
                                                return_counts=True, target_faces=cfg.get('spr_faces'), **_component_rules(cfg), **_smooth_rules(cfg))
        decimated = (f', decimated from {rc["faces_reconstructed"]} faces in {rc["simplify_rounds"]} rounds'
                     if 'simplify_rounds' in rc else '')
        logger.info(f'Get Geometry time: {time.time() - start} s by SPR (depth {depth}: {rc["vertices"]} vertices, {rc["faces"]} '
                    f'faces{decimated}, {rc["iterations"]} solver iterations; normals oriented by {rc["orientation"]})')
        if 'components' in rc:
            logger.info(f'SPR components: {rc["components"]} found, {rc["components_kept"]} kept, {rc["faces_dropped"]} of '
                        f'{rc["faces_reconstructed"]} reconstructed faces dropped')
        if 'smooth_steps' in rc:
            sm = _smooth_rules(cfg)['smooth']
            logger.info(f'SPR smoothing: {rc["smooth_steps"]} Taubin steps (lambda {sm["lam"]:g}, mu {sm["mu"]:g}): {rc["smooth_moved"]} vertices moved')
    if os.path.exists(geo_path) or os.path.exists(cached_geo):
        supplied = os.path.exists(geo_path)
        v, f, vt, ft = io_utils.load_obj_mesh(geo_path if supplied else cached_geo, with_uv=True)
        vertices = torch.from_numpy(v).to(device)
        faces = torch.from_numpy(f).to(device)
        if weld:
            vertices, faces, ft = _clean_supplied(cfg, vertices, faces, ft if vt is not None else None, logger)
        if orient:
            faces, ft = _orient_supplied(cfg, vertices, faces, ft if vt is not None else None, logger)
        if supplied:                                     # (the cached mesh was made from the normalised cloud: demo.py:401-406)
            vertices -= (vmax + vmin) / 2.
            vertices /= (vmax - vmin).max()
        if os.path.exists(xatlas_file):
            xatlas_dict = {k: (t.to(device) if torch.is_tensor(t) else t) for k, t in torch.load(xatlas_file).items()}
        elif vt is not None:
            # the mesh carries its UV parametrisation (`vt` + `f v/vt`): run the atlas producer (the rasterise + interpolate half of
            # xatlas_uvmap_w_face_id, extract_texture_map.py:48-64) and cache the dict in the reference's wire format (demo.py:445-448)
            from .extract_texture_map import uvmap_w_face_id
            uvs, tex_idx, gb_pos, amask, fid = uvmap_w_face_id(vertices, faces, torch.from_numpy(vt).to(device),
                                                               torch.from_numpy(ft).to(device), cfg.xatlas_texture_res)
            xatlas_dict = dict(uvs=uvs, mesh_tex_idx=tex_idx, gb_pos=gb_pos, mask=amask, per_atlas_pixel_face_id=fid)
            torch.save({k: t.cpu() for k, t in xatlas_dict.items()}, xatlas_file)
            logger.info(f'UV atlas rasterised from the mesh\'s own vt/f records -> {xatlas_file}')
        else:
            # no UVs (what POCO / SPR emit): unwrap on the device, then rasterise + interpolate, and cache the dict like the reference
            # does after xatlas_uvmap_w_face_id (demo.py:428-449)
            from .extract_texture_map import xatlas_uvmap_w_face_id
            logger.info('UV unwrapping...')
            start = time.time()
            uvs, tex_idx, gb_pos, amask, fid = xatlas_uvmap_w_face_id(None, vertices, faces, cfg.xatlas_texture_res)
            xatlas_dict = dict(uvs=uvs, mesh_tex_idx=tex_idx, gb_pos=gb_pos, mask=amask, per_atlas_pixel_face_id=fid)
            torch.save({k: t.cpu() for k, t in xatlas_dict.items()}, xatlas_file)
            logger.info(f'UV unwrapping time: {time.time() - start} s -> {xatlas_file}')
        logger.info('Existing geometry + xatlas data loaded')
    else:
        vertices, faces, xatlas_dict = standin_geometry(xyz, cfg.xatlas_texture_res, device, logger)
    f_normals = torch.from_numpy(synthetic.face_normals(vertices.cpu().numpy(), faces.cpu().numpy())).to(device)
    return dict(out=out, coords=xyz, colors=rgb, vertices=vertices, faces=faces, f_normals=f_normals, xatlas=xatlas_dict)


def _pipeline_kwargs(cfg):
    kw = {k: cfg[k] for k in SUPPORTED_KEYS if k in cfg and k != 'output_path'}
    kw.pop('camera_distribution', None)
    return kw


def recon_one_textured_mesh(cfg, inpainter, camera_info, pc_file, name, device, logger):
    """demo.py:359-466 (texturing part)."""
    all_start = time.time()
    sh = _load_shape(cfg, pc_file, name, device, logger)
    logger.info('Generate texture by PointDreamer...')
    start = time.time()
    vertices, uvs, faces, mesh_tex_idx, atlas_img, mask = pipeline.colorize_one_mesh(
        sh['coords'], sh['colors'], sh['vertices'], sh['faces'], sh['f_normals'], sh['xatlas'], camera_info, inpainter=inpainter,
        save_img_path=os.path.join(sh['out'], 'others'), device=device, logger=None, **_pipeline_kwargs(cfg))
    torch.cuda.synchronize()
    logger.info(f'generate texture time: {time.time() - start} s')
    save_textured_mesh(vertices, uvs, faces, mesh_tex_idx, atlas_img, mask, sh['out'])
    render_result(cfg, vertices, uvs, faces, mesh_tex_idx, atlas_img, sh['out'], device, logger)
    logger.info(f'total time: {time.time() - all_start} s')
    return sh['out']


def recon_textured_meshes_batched(cfg, inpainter, camera_info, pc_files, names, device, logger):
    """A directory run, several clouds at a time: the same stages and files as recon_one_textured_mesh per shape, with the views
    of all the shapes of the group in one inpainter batch (pipeline.colorize_meshes_batched)."""
    all_start = time.time()
    shapes = [_load_shape(cfg, pc, name, device, logger) for pc, name in zip(pc_files, names)]
    logger.info(f'Generate texture by PointDreamer ({len(shapes)} shapes in one batch)...')
    start = time.time()
    results = pipeline.colorize_meshes_batched(shapes, camera_info, inpainter=inpainter, return_full=True,
                                               save_img_paths=[os.path.join(sh['out'], 'others') for sh in shapes],
                                               **_pipeline_kwargs(cfg))
    torch.cuda.synchronize()
    logger.info(f'generate texture time: {time.time() - start} s ({(time.time() - start) / len(shapes)} s per shape)')
    for sh, (vertices, uvs, faces, mesh_tex_idx, atlas_img, mask) in zip(shapes, results):
        save_textured_mesh(vertices, uvs, faces, mesh_tex_idx, atlas_img, mask, sh['out'])
        render_result(cfg, vertices, uvs, faces, mesh_tex_idx, atlas_img, sh['out'], device, logger)
    logger.info(f'total time: {time.time() - all_start} s')
    return [sh['out'] for sh in shapes]


def recon_one_textured_mesh_view_parallel(cfg, inpainter, camera_info, pc_file, name, device, logger, rank, world, shape_key):
    """`--parallel views`: the views of ONE shape are split over the ranks (dist.colorize_one_mesh_view_parallel);
    every rank writes the per-view PNGs of its own views, rank 0 the mesh / atlas files."""
    from . import dist as pdist
    all_start = time.time()
    sh = _load_shape(cfg, pc_file, name, device, logger) if rank == 0 else None
    if world > 1:
        torch.distributed.barrier()                      # rank 0 created the output tree (input_pc.ply, geo cache) first
        if rank != 0:
            sh = _load_shape(cfg, pc_file, name, device, logger)
    logger.info(f'Generate texture by PointDreamer (views of the shape split over {world} ranks)...')
    start = time.time()
    vertices, uvs, faces, mesh_tex_idx, atlas_img, mask = pdist.colorize_one_mesh_view_parallel(
        sh['coords'], sh['colors'], sh['vertices'], sh['faces'], sh['f_normals'], sh['xatlas'], camera_info, rank=rank, world=world,
        inpainter=inpainter, save_img_path=os.path.join(sh['out'], 'others'), shape_key=shape_key, return_full=True,
        **_pipeline_kwargs(cfg))
    torch.cuda.synchronize()
    logger.info(f'generate texture time: {time.time() - start} s')
    if rank == 0:
        save_textured_mesh(vertices, uvs, faces, mesh_tex_idx, atlas_img, mask, sh['out'])
        render_result(cfg, vertices, uvs, faces, mesh_tex_idx, atlas_img, sh['out'], device, logger)
    logger.info(f'total time: {time.time() - all_start} s')
    return sh['out']


def files_of_rank(pc_files, rank, world):
    """The clouds rank `rank` of `world` textures: a contiguous block of the sorted list (dist.shard_range)."""
    from .dist import shard_range
    return [pc_files[i] for i in shard_range(len(pc_files), rank, world)]


def main(argv=None):
    p = argparse.ArgumentParser("PointDreamer (MI355X texturing path)")
    p.add_argument("--config", type=str, default='configs/default.yaml', help="path to config file")
    p.add_argument("--pc_file", type=str, default='dataset/demo_data/clock.ply', help="path to input point cloud file or directory")
    p.add_argument("--ckpt", type=str, default=None, help="256x256_diffusion_uncond.pt (reference key names)")
    p.add_argument("--allow_random_weights", action='store_true', help="run DDNM with random-init weights if the checkpoint is absent")
    p.add_argument("--set", nargs='*', default=[], help="YAML overrides key=value (e.g. complete_unseen_by=unproject optimize_from=None)")
    p.add_argument("--batch_shapes", type=int, default=4, help="directory runs: clouds textured together, their views in one "
                   "inpainter batch (1 = one at a time, as the reference -- the only route that re-uses existing {k}_inpainted.png "
                   "files of a resumed output directory, demo.py:138-147; 4 is ~16 %% more shapes/hour on one MI355X)")
    p.add_argument("--parallel", choices=['shapes', 'views'], default='shapes', help="under torch.distributed.run: 'shapes' = every "
                   "rank textures its own block of the clouds (no collective); 'views' = the views of each shape are split over the "
                   "ranks and assembled with one all_gather (lowest latency per shape; needs world size <= view_num)")
    args = p.parse_args(argv)
    # Host threads: torch sizes its intra-op pool by the machine's logical CPUs (256 on the pool's boxes) while the container's cgroup
    # grants 16 -- a 128-thread OpenMP region around a 90 000-element `.float()` next to the PNG-encoder threads exhausts the CFS quota
    # and the whole process is throttled for the rest of the period (round 5: 99 ms per `_load_shape` in a directory run against 2.5 ms
    # alone).  The CLI's CPU tensors are small: a few threads, inside the quota.
    torch.set_num_threads(max(1, min(4, io_utils.cpus_per_rank() // 4)))
    # one process per GPU (`python -m torch.distributed.run --nproc-per-node N -m pointdreamer_amd.demo ...`): every rank textures its
    # own contiguous block of the directory's clouds -- independent shapes, no collective on the data path
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0))) if world > 1 else torch.device('cuda')
    if world > 1:
        torch.cuda.set_device(device)
    overrides = {k: yaml.safe_load(v) for k, v in (kv.split('=', 1) for kv in args.set)}
    pc_files = [args.pc_file] if args.pc_file.endswith('.ply') else \
        [os.path.join(args.pc_file, i) for i in sorted(os.listdir(args.pc_file)) if i.endswith('.ply')]
    by_views = args.parallel == 'views' and world > 1
    if by_views:
        import torch.distributed as tdist
        if not tdist.is_initialized():
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            tdist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)
    else:
        pc_files = files_of_rank(pc_files, rank, world)
    group = 1 if by_views else max(1, min(args.batch_shapes, max(1, len(pc_files))))
    cfg, inpainter, camera_info, logger = prepare(args.config, device, args.ckpt, args.allow_random_weights, overrides, batch_shapes=group)
    outs = []
    # PNG / OBJ encoding of one shape runs on host threads under the GPU work of the next (io_utils.set_async); every file is on
    # disk when main() returns
    io_utils.set_async(True, workers=max(2, min(8, io_utils.cpus_per_rank() - 4)))
    try:
        for g0 in range(0, len(pc_files), group):
            chunk = pc_files[g0:g0 + group]
            names = [os.path.basename(f).split('.ply')[0] + '_' + os.path.basename(args.config).split('.')[0] for f in chunk]
            for pc_file, name in zip(chunk, names):
                os.makedirs(os.path.join(cfg.output_path, name), exist_ok=True)
                shutil.copy(args.config, os.path.join(cfg.output_path, name, 'config.yaml'))
                logger.info(f'Start Recon {pc_file}...')
            if by_views:
                outs.append(recon_one_textured_mesh_view_parallel(cfg, inpainter, camera_info, chunk[0], names[0], device, logger,
                                                                  rank, world, shape_key=g0))
            elif len(chunk) == 1:
                outs.append(recon_one_textured_mesh(cfg, inpainter, camera_info, chunk[0], names[0], device, logger))
            else:
                outs += recon_textured_meshes_batched(cfg, inpainter, camera_info, chunk, names, device, logger)
    finally:
        io_utils.set_async(False)          # flushes
    return outs


if __name__ == '__main__':
    main()
