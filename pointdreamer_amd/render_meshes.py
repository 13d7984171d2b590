"""data/render_meshes.py of the reference: render every mesh below <rootpath>/meshes into <rootpath>/rendered_imgs.

    - rootpath
        - meshes / cls_id / shape_name / models / model_normalized.obj (+ .mtl, .png)
        - rendered_imgs / cls_id / shape_name / albedo_0XX.png          (XX from 01 to 20, RGBA, 1024 x 1024)

  python -m pointdreamer_amd.render_meshes --rootpath <rootpath> --by kaolin|kaolin_per_vertex

`--by` keeps the reference's two values: 'kaolin' renders textured OBJ files -- one material or several, `map_Kd` images of any size
next to plain `Kd` colours, the material of the face chosen per pixel -- and 'kaolin_per_vertex' OBJ files with `v x y z r g b`
records; both run on this build's device rasteriser and shading kernels (kaolin and nvdiffrast are not dependencies)."""
import argparse

import torch

from . import io_utils
from .camera_utils import render_textured_meshes_shapenet2


def main(argv=None):
    p = argparse.ArgumentParser("render meshes")
    p.add_argument("--rootpath", type=str, default='', help="path to the root path of meshes to be rendered")
    p.add_argument("--by", type=str, default='kaolin', choices=['kaolin', 'kaolin_per_vertex'], help="kaolin or kaolin_per_vertex")
    args = p.parse_args(argv)
    device = torch.device('cuda')
    io_utils.set_async(True, workers=max(2, min(8, io_utils.cpus_per_rank() - 4)))
    try:
        n = render_textured_meshes_shapenet2(root_path=args.rootpath, device=device, per_vertex=args.by == 'kaolin_per_vertex')
    finally:
        io_utils.set_async(False)
    print(f'{n} shapes rendered under {args.rootpath}/rendered_imgs')
    return n


if __name__ == '__main__':
    main()
