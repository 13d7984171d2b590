"""data/sample_colored_pc_from_mesh.py of the reference on the MI355X: textured ground-truth meshes -> the <= 30 k-point coloured
clouds the texturing path, the renderer and the evaluation consume.  Same function names and call shapes; kaolin's OBJ importer,
face_areas + sample_points, the per-material grid_sample loop and the nvdiffrast depth test are replaced by a multi-material OBJ
loader on the host, ONE kernel call (pdhip_sample_mesh, csrc/sample_mesh.hip) and the texturing path's own visibility stages.

Deviations from the reference, all deliberate:
  * the draw is a deterministic function of explicit uniforms (`rand`, or a torch generator): kaolin's Categorical / torch.rand stream
    and numpy's shuffle are not reproduced; the face is chosen through an exact integer CDF (include/pdhip.h);
  * `face_idx` always indexes the mesh's own face list (with face_visibility the reference indexes the filtered list next to normals
    of the unfiltered one), and face_idx.npy is int32 (the reference casts to uint8 and wraps at 256);
  * too few visible points raise ValueError with both counts (the reference asserts);
  * the caller's vertices are never modified (the reference normalises them in place).

  python -m pointdreamer_amd.sample_colored_pc_from_mesh --rootpath ROOT [--cls_id ...] [--point_num 30000] [--seed 0] [--ply]
  python -m pointdreamer_amd.sample_colored_pc_from_mesh --rootpath ROOT [--cls_id ...] --occupancy [N] [--padding 0.1] [--seed 0]

The second form (sample_occupancy_batch) writes no clouds: it tests N uniform points against every mesh on the device and stores them
with their occupancies as <ROOT>/point/<cls_id>/<name>.npz, the ground truth of the volumetric IoU (geometry_metrics.eval_mesh).
"""
import argparse
import logging
import os
import sys
import traceback
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream, check

NPY_FILES = ('coords.npy', 'colors.npy', 'normals.npy', 'uvs.npy', 'material_idx.npy', 'face_idx.npy')
MAX_MATERIALS = 255                                  # material_idx.npy is uint8, as the reference saves it
DEFAULT_KD = (0.5, 0.5, 0.5)


# ----------------------------------------------------------------------------- loader (kal.io.obj.import_mesh(with_materials=True))
class MeshData:
    """What load_obj_with_materials returns, plus `name` ('<cls_id>/<name>').  `.data` and `.attributes['name']` are the two
    accessors the reference uses on its KaolinDatasetItem."""

    def __init__(self, vertices, faces, uvs, face_uvs_idx, face_material, materials, name=''):
        self.vertices, self.faces, self.uvs, self.face_uvs_idx = vertices, faces, uvs, face_uvs_idx
        self.face_material, self.materials, self.name = face_material, materials, name
        self.attributes = {'name': name}

    @property
    def data(self):
        return self


def load_obj_with_materials(mesh_file):
    """vertices [Vn,3] f32, faces [F,3] i64, vt [T,2] f32, per-corner vt indices [F,3] i64 (-1 where the record has none), per-face
    material index [F] i32 and the material list -- one dict per `newmtl` in MTL order with 'name' and either 'map_Kd' (uint8
    [H,W,3], opened with PIL and converted to RGB, rows as the file stores them) or 'Kd' (float32 [3]).  Polygons are
    fan-triangulated as io_utils.load_obj_mesh does; `usemtl` maps by name.  A mesh without an MTL (or whose MTL defines nothing)
    gets one grey Kd material.  ValueError naming the file: a `usemtl` of an unknown material, a face before the first `usemtl`
    while the MTL defines materials, more than 255 materials."""
    import PIL.Image
    from .camera_utils import _load_mtl
    here = os.path.dirname(mesh_file)
    vs, vts, fs, fts, fms = [], [], [], [], []
    mats, by_name, cur = [], {}, -1
    with open(mesh_file) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == 'v':
                vs.append([float(x) for x in t[1:4]])
            elif t[0] == 'vt':
                vts.append([float(x) for x in t[1:3]])
            elif t[0] == 'mtllib' and len(t) > 1:
                for name, m in _load_mtl(os.path.join(here, line.split(None, 1)[1].strip())):
                    if name not in by_name:
                        by_name[name] = len(mats)
                        mats.append((name, m))
                if len(mats) > MAX_MATERIALS:
                    raise ValueError(f"{mesh_file}: {len(mats)} materials, more than {MAX_MATERIALS}")
            elif t[0] == 'usemtl' and mats:
                name = t[1] if len(t) > 1 else ''
                if name not in by_name:
                    raise ValueError(f"{mesh_file}: usemtl {name!r} names no material of the MTL")
                cur = by_name[name]
            elif t[0] == 'f':
                if mats and cur < 0:
                    raise ValueError(f"{mesh_file}: a face precedes the first usemtl although the MTL defines {len(mats)} material(s)")
                parts = [x.split('/') for x in t[1:]]
                idx = [int(p[0]) for p in parts]
                idx = [i - 1 if i > 0 else len(vs) + i for i in idx]
                tix = [int(p[1]) if len(p) > 1 and p[1] else 0 for p in parts]
                tix = [i - 1 if i > 0 else (len(vts) + i if i < 0 else -1) for i in tix]
                for k in range(1, len(idx) - 1):
                    fs.append([idx[0], idx[k], idx[k + 1]])
                    fts.append([tix[0], tix[k], tix[k + 1]])
                    fms.append(max(cur, 0))
    materials = []
    for name, m in mats:
        if 'map_Kd' in m:
            im = PIL.Image.open(os.path.join(here, m['map_Kd'])).convert('RGB')
            materials.append({'name': name, 'map_Kd': np.ascontiguousarray(np.asarray(im, np.uint8))})
        else:
            materials.append({'name': name, 'Kd': np.asarray(m.get('Kd', DEFAULT_KD), np.float32).reshape(3)})
    if not materials:
        materials = [{'name': '', 'Kd': np.asarray(DEFAULT_KD, np.float32)}]
    return (np.array(vs, np.float32).reshape(-1, 3), np.array(fs, np.int64).reshape(-1, 3), np.array(vts, np.float32).reshape(-1, 2),
            np.array(fts, np.int64).reshape(-1, 3), np.array(fms, np.int32), materials)


def pack_materials(materials, device):
    """The material set as the kernel takes it: texels (uint8, every image's RGB bytes one after the other, rows as stored),
    mat_offset [M] i64 (first byte of material m's image), mat_wh [M,2] i32 ((W, H); (0, 0) = no image) and mat_kd [M,3] f32 (the
    colour of a material without an image)."""
    if not materials:
        raise ValueError("pack_materials: empty material list")
    chunks, off, wh, kd, total = [], [], [], [], 0
    for m in materials:
        img = m.get('map_Kd') if isinstance(m, dict) else None
        off.append(total)
        if img is not None:
            img = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
                raise ValueError(f"pack_materials: map_Kd must be uint8 [H,W,3], got {img.dtype} {img.shape}")
            chunks.append(np.ascontiguousarray(img).reshape(-1))
            wh.append([img.shape[1], img.shape[0]])
            kd.append([0.0, 0.0, 0.0])
            total += img.size
        else:
            c = m['Kd'] if isinstance(m, dict) else m
            c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
            wh.append([0, 0])
            kd.append(np.asarray(c, np.float32).reshape(3).tolist())
    texels = np.concatenate(chunks) if chunks else np.zeros((0,), np.uint8)
    return (torch.from_numpy(texels).to(device), torch.tensor(off, dtype=torch.int64, device=device),
            torch.tensor(wh, dtype=torch.int32, device=device).reshape(-1, 2), torch.tensor(kd, dtype=torch.float32, device=device).reshape(-1, 3))


# ----------------------------------------------------------------------------- the kernel call
def _on(x, dev, dtype):
    if x is None:
        return None
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return x.to(device=dev, dtype=dtype).contiguous()


def sample_points(vertices, faces, uvs, face_uvs_idx, face_material, materials, num_samples, face_keep=None, rand=None, generator=None):
    """pdhip_sample_mesh on tensors (include/pdhip.h has the contract): vertices [Vn,3] on the GPU, faces [F,3], uvs [T,2] with
    face_uvs_idx [F,3] (-1: that corner's UV is (0,0); both may be None), face_material [F] (None: material 0), materials (the list
    load_obj_with_materials returns, or the four tensors of pack_materials), face_keep [F] bool (None: every face) -> dict with the
    reference's keys: coords [N,3], face_idx [N] i32 (into `faces`), material_idx [N] i32, uvs [N,2] (before the wrap), colors
    [N,3] in [0,1], normals [N,3].  `rand` [N,3] in [0,1) are the uniforms (face, u, v); default torch.rand from `generator`."""
    L = _lib.lib()
    if not (torch.is_tensor(vertices) and vertices.is_cuda):
        raise _lib.PdhipError("sample_points: expected vertices on the GPU; pointdreamer_amd has no CPU path")
    dev, N = vertices.device, int(num_samples)
    vertices = vertices.detach().float().contiguous()
    faces = _on(faces, dev, torch.int64)
    uvs, face_uvs_idx = _on(uvs, dev, torch.float32), _on(face_uvs_idx, dev, torch.int64)
    if uvs is None or face_uvs_idx is None or uvs.numel() == 0:
        if face_uvs_idx is not None and uvs is not None and bool((face_uvs_idx >= 0).any()):
            raise _lib.PdhipError("sample_points: face_uvs_idx refers to an empty uv table")
        uvs = face_uvs_idx = None
    face_material = _on(face_material, dev, torch.int32)
    keep = _on(face_keep, dev, torch.bool)
    texels, mat_offset, mat_wh, mat_kd = (tuple(_on(t, dev, t.dtype) for t in materials) if isinstance(materials, tuple)
                                          else pack_materials(materials, dev))
    if rand is None:
        on_host = generator is not None and generator.device.type != dev.type          # (a CPU generator draws on the host)
        rand = torch.rand((N, 3), device=generator.device if on_host else dev, generator=generator)
    rand = _on(rand, dev, torch.float32)
    if tuple(rand.shape) != (N, 3):
        raise _lib.PdhipError(f"sample_points: rand must be [{N}, 3], got {tuple(rand.shape)}")
    Vn, F, T, M = vertices.shape[0], faces.shape[0], 0 if uvs is None else uvs.shape[0], mat_offset.shape[0]
    out = dict(coords=torch.empty((N, 3), device=dev), face_idx=torch.empty((N,), dtype=torch.int32, device=dev),
               material_idx=torch.empty((N,), dtype=torch.int32, device=dev), uvs=torch.empty((N, 2), device=dev),
               colors=torch.empty((N, 3), device=dev), normals=torch.empty((N, 3), device=dev))
    ws = torch.empty((max(int(L.pdhip_sample_mesh_workspace_bytes(F, N)), 8),), dtype=torch.uint8, device=dev)   # (0: the entry refuses F)
    opt = lambda t, dt=None: ptr(t, dt, allow_none=True) if t is not None and t.numel() else ptr(None, allow_none=True)
    check(L.pdhip_sample_mesh(ptr(vertices, torch.float32), Vn, ptr(faces), F, opt(uvs), T, opt(face_uvs_idx), opt(face_material),
                              opt(None if keep is None else _lib.as_u8(keep)), opt(texels, torch.uint8), int(texels.numel()),
                              ptr(mat_offset, torch.int64), ptr(mat_wh, torch.int32), ptr(mat_kd, torch.float32), M, opt(rand), N,
                              opt(out['coords']), opt(out['colors']), opt(out['normals']), opt(out['uvs']), opt(out['face_idx']),
                              opt(out['material_idx']), ptr(ws), stream()), 'pdhip_sample_mesh')
    return out


# ----------------------------------------------------------------------------- the reference's transforms
def preprocessing_transform(inputs, face_visibility=None):
    """:50-128.  The areas, the diffuse maps and the per-face materials of the reference's dict are computed inside the kernel; what
    is left is to name the tensors.  `face_visibility` [F] bool drops faces from the draw (their indices stay those of the mesh)."""
    mesh = inputs.data
    return {'vertices': mesh.vertices, 'faces': mesh.faces, 'uvs': mesh.uvs, 'face_uvs_idx': mesh.face_uvs_idx,
            'face_material_idx': mesh.face_material, 'materials': mesh.materials, 'face_keep': face_visibility,
            'name': inputs.attributes['name']}


class SamplePointsTransform(object):
    """:132-184: `num_samples` coloured points of a preprocessing_transform dict, on the device the vertices live on (CUDA; host
    arrays are moved to `device`)."""

    def __init__(self, num_samples, device=None, generator=None, rand=None):
        self.num_samples, self.device, self.generator, self.rand = num_samples, device, generator, rand

    def __call__(self, inputs):
        v = inputs['vertices']
        if not (torch.is_tensor(v) and v.is_cuda):
            v = _on(v, _lib.resolve_device(self.device if self.device is not None else 'cuda'), torch.float32)
        out = sample_points(v, inputs['faces'], inputs['uvs'], inputs['face_uvs_idx'], inputs['face_material_idx'], inputs['materials'],
                            self.num_samples, face_keep=inputs.get('face_keep'), rand=self.rand, generator=self.generator)
        out['name'] = inputs['name']
        return out


def sample_pc(mesh_data, point_num=30000, face_visibility=None, device=None, generator=None):
    """:275-292 -> (coords, colors, normals, material_idx, face_idx, uvs) as numpy arrays."""
    out = SamplePointsTransform(point_num, device=device, generator=generator)(preprocessing_transform(mesh_data, face_visibility))
    return tuple(out[k].cpu().numpy() for k in ('coords', 'colors', 'normals', 'material_idx', 'face_idx', 'uvs'))


def visible_point_mask(vertices, faces, points, cameras):
    """[N] bool: the point passes the depth test (point depth <= mesh depth at its pixel, offset 0) in at least one view.  A
    composition of the texturing path's stages: pdhip_project_points with rescale = 0, the rasteriser's depth image,
    pdhip_point_visibility, an OR over the views."""
    from . import ours_utils as ou
    res = int(cameras[0].height)
    _, _, depth, _, _, _, _, puv, pdep = ou.get_rendered_hard_mask_and_face_idx_batch(cameras, vertices, faces, points, None, False, 0)
    vis, _ = ou.get_point_validation_by_depth(res, puv, pdep, depth, offset=0)
    return vis.any(0)


def sample_one_mesh_w_o_invisible_points(mesh_data, point_per_shape, cameras, device, save_root, generator=None):
    """:295-388: normalise a COPY of the vertices to the unit box, draw 5 * point_per_shape samples, keep the points that pass the
    depth test in at least one of `cameras`, take a random subset of point_per_shape of them (torch.randperm on `generator`, left
    in that random order) and save the six .npy files under <save_root>/<cls>/<name>/ (save_root None: nothing is written).
    Returns the reference's tuple (coords, colors, material_idx, face_idx, uvs) as numpy arrays.  Fewer visible points than
    point_per_shape: ValueError with both counts.

    The depth test is visible_point_mask.  Its pixel rule is the texturing path's, clip(uv * res) truncated with uv = (xy + 1) / 2;
    the reference's sampler computes xy * res / 2 + res / 2 instead.  The two agree except where float32 rounding puts a point on
    a pixel edge."""
    from .camera_utils import _normalized
    dev = _lib.resolve_device(device)
    mesh = mesh_data.data
    vertices = _normalized(_on(mesh.vertices, dev, torch.float32)).contiguous()          # (a new tensor)
    faces = _on(mesh.faces, dev, torch.int64)
    n_draw = 5 * int(point_per_shape)
    s = sample_points(vertices, faces, mesh.uvs, mesh.face_uvs_idx, mesh.face_material, mesh.materials, n_draw, generator=generator)
    kept = torch.nonzero(visible_point_mask(vertices, faces, s['coords'], cameras)).reshape(-1)
    if kept.numel() < point_per_shape:
        raise ValueError(f"{mesh_data.attributes['name']}: {kept.numel()} of {n_draw} samples are visible, fewer than the "
                         f"{point_per_shape} points asked for")
    gdev = generator.device if generator is not None else dev
    sel = kept[torch.randperm(kept.numel(), generator=generator, device=gdev)[:point_per_shape].to(dev)]
    outputs = {k: s[k][sel].cpu().numpy() for k in ('coords', 'face_idx', 'material_idx', 'uvs', 'colors', 'normals')}
    outputs['name'] = mesh_data.attributes['name']
    if save_root is not None:
        save_one_mesh_npy(outputs, save_root=save_root)
    return outputs['coords'], outputs['colors'], outputs['material_idx'], outputs['face_idx'], outputs['uvs']


# ----------------------------------------------------------------------------- files
def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def save_one_mesh_npy(inputs, save_root):
    """:187-222: <save_root>/<cls>/<name>/{coords f4, colors u8 = (c * 255) truncated, normals f4, uvs f4, material_idx u8,
    face_idx i4}.npy.  (The reference stores face_idx as uint8, which wraps at 256.)"""
    cls_id, mesh_id = inputs['name'].split('/')
    save_path = os.path.join(save_root, cls_id, mesh_id)
    os.makedirs(save_path, exist_ok=True)
    np.save(os.path.join(save_path, 'coords.npy'), _np(inputs['coords']).astype('f4'))
    np.save(os.path.join(save_path, 'colors.npy'), (_np(inputs['colors']) * 255).astype('uint8'))
    np.save(os.path.join(save_path, 'normals.npy'), _np(inputs['normals']).astype('f4'))
    np.save(os.path.join(save_path, 'uvs.npy'), _np(inputs['uvs']).astype('f4'))
    np.save(os.path.join(save_path, 'material_idx.npy'), _np(inputs['material_idx']).astype('uint8'))
    np.save(os.path.join(save_path, 'face_idx.npy'), _np(inputs['face_idx']).astype('i4'))
    return save_path


def load_pc_npy(filedir):
    """:582-588 -> coords, colors (uint8), material_idx, face_idx, uvs."""
    ld = lambda n: np.load(os.path.join(filedir, n))
    return ld('coords.npy'), ld('colors.npy'), ld('material_idx.npy'), ld('face_idx.npy'), ld('uvs.npy')


# ----------------------------------------------------------------------------- datasets
def _mesh_data(mesh_file, cls_id, name):
    return MeshData(*load_obj_with_materials(mesh_file), name=f'{cls_id}/{name}')


def get_other_mesh_data(root_path, name, cls_id='google_scanned_objects'):
    """:404-414: <root_path>/meshes/<cls_id>/<name>/ in any of the four layouts camera_utils._find_mesh_file knows."""
    from .camera_utils import _find_mesh_file
    return _mesh_data(_find_mesh_file(root_path, cls_id, name), cls_id, name)


def get_shapenet2_mesh_data(shapenet_clean_root_path, cls_id, name):
    """:398-402: `shapenet_clean_root_path` is the `meshes` directory itself (<root>/meshes/<cls_id>/<name>/models/...)."""
    root = os.path.normpath(shapenet_clean_root_path)
    if os.path.basename(root) == 'meshes':
        return get_other_mesh_data(os.path.dirname(root), name, cls_id)
    return _mesh_data(os.path.join(root, cls_id, name, 'models', 'model_normalized.obj'), cls_id, name)


def _sample_batch(root_path, cls_ids=None, point_num=30000, seed=0, ply=False, device=None):
    """Every <root_path>/meshes/<cls>/<name> -> <root_path>/pc_kaolin/<cls>/<name>/*.npy (and <cls>/<name>.ply with `ply`), through the
    20 cameras of the reference (:30).  A shape whose six files exist is skipped; a shape that fails is logged with its traceback
    and the run goes on.  Each shape's uniforms come from a generator seeded by (seed, crc32 of '<cls>/<name>'), so a resumed run
    writes what an uninterrupted one would.  Returns the number of shapes sampled."""
    from .camera_utils import create_cameras
    from . import io_utils
    dev = _lib.resolve_device(device if device is not None else 'cuda')
    log = logging.getLogger('pointdreamer_amd.sample_pc')
    cameras, _, _, _ = create_cameras(num_views=20, distance=1.6, res=256, device=dev)
    save_root = os.path.join(root_path, 'pc_kaolin')
    mesh_root = os.path.join(root_path, 'meshes')
    if cls_ids is None:
        cls_ids = [c for c in sorted(os.listdir(mesh_root)) if os.path.isdir(os.path.join(mesh_root, c))]
    done = 0
    for cls_id in cls_ids:
        names = sorted(n for n in os.listdir(os.path.join(mesh_root, cls_id)) if os.path.isdir(os.path.join(mesh_root, cls_id, n)))
        for i, name in enumerate(names):
            out_dir = os.path.join(save_root, cls_id, name)
            ply_file = os.path.join(save_root, cls_id, name + '.ply')
            if all(os.path.exists(os.path.join(out_dir, f)) for f in NPY_FILES) and (not ply or os.path.exists(ply_file)):
                log.info(f'skip exist {out_dir}')
                continue
            log.info(f'{i}/{len(names)}:{cls_id}/{name}')
            try:
                gen = torch.Generator().manual_seed((int(seed) << 32) ^ zlib.crc32(f'{cls_id}/{name}'.encode()))
                mesh_data = get_other_mesh_data(root_path, name, cls_id=cls_id)
                coords, colors, _, _, _ = sample_one_mesh_w_o_invisible_points(mesh_data, point_num, cameras, dev, save_root, generator=gen)
                if ply:
                    io_utils.save_colored_pc_ply(coords, colors, ply_file)
                done += 1
            except KeyboardInterrupt:
                raise
            except Exception:                      # noqa: BLE001 -- the reference logs the shape and goes on (:440-441)
                log.error(f'{i},{cls_id}/{name}')
                log.error(traceback.format_exc())
    return done


def sample_shapenet_core_v2_mesh_batch(root_path, cls_ids=None, point_num=30000, seed=0, ply=False, device=None):
    """:416-441 over <root_path>/meshes/<synset>/<model>/models/model_normalized.obj; `cls_ids` None: every synset there."""
    return _sample_batch(root_path, cls_ids, point_num, seed, ply, device)


def sample_google_scanned_objects_batch(root_path='datasets/google_scanned_objects', cls_id='google_scanned_objects', point_num=30000,
                                        seed=0, ply=False, device=None):
    """:444-463."""
    return _sample_batch(root_path, [cls_id], point_num, seed, ply, device)


def sample_omniobject3d_batch(root_path='datasets/omniobject3d', cls_id='omniobject3d', point_num=30000, seed=0, ply=False, device=None):
    """:465-484."""
    return _sample_batch(root_path, [cls_id], point_num, seed, ply, device)


def sample_occupancy_batch(root_path, cls_ids=None, n_points=100000, padding=0.1, seed=0, device=None):
    """Every <root_path>/meshes/<cls>/<name> -> <root_path>/point/<cls>/<name>.npz with `points` (float32 [n_points,3]) and `occupancies`
    (np.packbits of the [n_points] inside / outside flags): the two keys the reference's loader reads (models/POCO/datasets/shapenet.py:200-203)
    as the ground truth of eval_mesh's `iou`.  The mesh is normalised as the point sampler normalises it (camera_utils._normalized); the
    points are uniform in [-(1 + padding) / 2, (1 + padding) / 2]^3 -- the box is this project's choice, the convention of Occupancy
    Networks, not something the reference fixes: it reads such files and does not write them --, drawn as float32 from the generator
    seeded by (seed, crc32 of '<cls>/<name>') that _sample_batch uses, and tested as the float32 values that are stored
    (geometry_metrics.check_mesh_contains, the reference's check_mesh_contains on the device).  A shape whose file exists is skipped; a
    shape that fails is logged with its traceback and the run goes on.  Per shape the number of points whose two ray parities disagree is
    logged: a mesh that is not closed gets the reference's conservative answer there (not contained), which is the reference's
    behaviour and not an error.  Returns the number of files written."""
    from .camera_utils import _normalized
    from .geometry_metrics import check_mesh_contains
    dev = _lib.resolve_device(device if device is not None else 'cuda')
    log = logging.getLogger('pointdreamer_amd.sample_pc')
    save_root = os.path.join(root_path, 'point')
    mesh_root = os.path.join(root_path, 'meshes')
    if cls_ids is None:
        cls_ids = [c for c in sorted(os.listdir(mesh_root)) if os.path.isdir(os.path.join(mesh_root, c))]
    half = (1.0 + float(padding)) / 2.0
    done = 0
    for cls_id in cls_ids:
        names = sorted(n for n in os.listdir(os.path.join(mesh_root, cls_id)) if os.path.isdir(os.path.join(mesh_root, cls_id, n)))
        for i, name in enumerate(names):
            out_file = os.path.join(save_root, cls_id, name + '.npz')
            if os.path.exists(out_file):
                log.info(f'skip exist {out_file}')
                continue
            log.info(f'{i}/{len(names)}:{cls_id}/{name}')
            try:
                gen = torch.Generator().manual_seed((int(seed) << 32) ^ zlib.crc32(f'{cls_id}/{name}'.encode()))
                mesh = get_other_mesh_data(root_path, name, cls_id=cls_id).data
                vertices = _normalized(_on(mesh.vertices, dev, torch.float32)).contiguous()
                points = ((torch.rand((int(n_points), 3), generator=gen) * 2.0 - 1.0) * half).to(torch.float32).contiguous()
                occ, counts = check_mesh_contains(vertices, _on(mesh.faces, dev, torch.int64), points.to(dev), return_counts=True)
                contained, disagree, outside, _ = counts.cpu().tolist()
                log.info(f'{cls_id}/{name}: {contained} of {int(n_points)} points inside, {outside} outside the box of the mesh, '
                         f'{disagree} with disagreeing parities (taken as outside)')
                os.makedirs(os.path.dirname(out_file), exist_ok=True)
                np.savez(out_file, points=points.numpy(), occupancies=np.packbits(occ.cpu().numpy()))
                done += 1
            except KeyboardInterrupt:
                raise
            except Exception:                      # noqa: BLE001 -- as _sample_batch: log the shape and go on
                log.error(f'{i},{cls_id}/{name}')
                log.error(traceback.format_exc())
    return done


def main(argv=None):
    p = argparse.ArgumentParser(description="Sample coloured point clouds from <rootpath>/meshes/<cls_id>/<name> into <rootpath>/pc_kaolin")
    p.add_argument('--rootpath', required=True)
    p.add_argument('--cls_id', nargs='*', default=None, help="class folders under <rootpath>/meshes (default: all)")
    p.add_argument('--point_num', type=int, default=30000)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--ply', action='store_true', help="also write <cls_id>/<name>.ply (xyz + rgb), the input of demo --pc_file")
    p.add_argument('--occupancy', type=int, nargs='?', const=100000, default=None, metavar='N',
                   help="instead of the clouds, write <rootpath>/point/<cls_id>/<name>.npz: N (default 100000) points in the padded unit box "
                        "and their inside / outside flags, the ground truth of run_geometry_evaluation's iou")
    p.add_argument('--padding', type=float, default=0.1, help="with --occupancy: the points fill [-(1 + padding) / 2, (1 + padding) / 2]^3")
    args = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(levelname)s %(message)s')
    if args.occupancy is not None:
        done = sample_occupancy_batch(args.rootpath, args.cls_id or None, args.occupancy, args.padding, args.seed)
        print(f'wrote the occupancies of {done} shape(s) into {os.path.join(args.rootpath, "point")}')
        return 0
    done = _sample_batch(args.rootpath, args.cls_id or None, args.point_num, args.seed, args.ply)
    print(f'sampled {done} shape(s) into {os.path.join(args.rootpath, "pc_kaolin")}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
