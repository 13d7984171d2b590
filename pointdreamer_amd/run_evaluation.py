"""data/run_evaluation.py of the reference, PSNR and SSIM on the device:

  python -m pointdreamer_amd.run_evaluation --pred_root_path <pred>/rendered_imgs --gt_root_path <gt>/rendered_imgs

Both roots hold <cls_id>/<shape_name>/albedo_%03d.png (or color_%03d.png); every shape of the prediction root is compared view by
view with the shape of the same name.  Images are read as run_evaluation.py:23-37 reads them (RGBA, transparent pixels become
(0,255,0)) and resized to `--rendered_img_res` when their size differs.  The score is the mean over the views of a shape, then the
mean over the shapes; the reference's result line goes to `<parent of pred root>/<time>_eval_result.txt`.  FID and LPIPS need networks
this project does not ship: they are reported as -100, the reference's "not computed" value."""
import argparse
import os
import time

import numpy as np
import torch

from . import metric_utils

NOT_COMPUTED = -100


def imread(filename, background=(0, 255, 0)):
    """run_evaluation.py:23-37 up to the division: (height, width, 3) uint8, transparent pixels set to `background`."""
    import PIL.Image
    rgba = np.array(PIL.Image.open(filename).convert('RGBA'), dtype=np.uint8)
    img = rgba[..., :3].copy()
    if background is not None:
        img[rgba[..., 3] == 0] = background
    return img


def _view_path(root, name, view_id, first, second):
    p = os.path.join(root, name, '{:s}_{:03d}.png'.format(first, view_id + 1))
    return p if os.path.exists(p) else os.path.join(root, name, '{:s}_{:03d}.png'.format(second, view_id + 1))


def load_views(root, name, view_num, res, first, second, device):
    """uint8 [view_num,res,res,3] on the device (run_evaluation.py:67-101; the reference resizes the float image with torchvision's
    Resize -- bilinear, antialiased -- and rounds back to 8 bits, :94-96, :227)."""
    out = torch.empty((view_num, res, res, 3), dtype=torch.uint8)
    for v in range(view_num):
        img = torch.from_numpy(imread(_view_path(root, name, v, first, second)))
        if img.shape[0] != res or img.shape[1] != res:
            f = torch.nn.functional.interpolate((img.permute(2, 0, 1)[None].double() / 255.0), size=(res, res), mode='bilinear',
                                                align_corners=False, antialias=True)
            img = (f[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8)
        out[v] = img
    return out.to(device)


def shape_names(pred_root_path):
    names = []
    for cls_id in sorted(os.listdir(pred_root_path)):
        d = os.path.join(pred_root_path, cls_id)
        if os.path.isdir(d):
            names += [f'{cls_id}/{n}' for n in sorted(os.listdir(d)) if os.path.isdir(os.path.join(d, n))]
    return names


def eval(pred_root_path, gt_root_path, view_num=20, rendered_img_res=512, device=None):
    """Returns dict(fid, lpips, psnr, ssim, sample_num, result_file)."""
    device = device if device is not None else torch.device('cuda')
    names = shape_names(pred_root_path)
    if not names:
        raise FileNotFoundError(f'no <cls_id>/<shape_name> directories under {pred_root_path}')
    psnrs, ssims = [], []
    for name in names:
        gt = load_views(gt_root_path, name, view_num, rendered_img_res, 'color', 'albedo', device)
        pred = load_views(pred_root_path, name, view_num, rendered_img_res, 'albedo', 'color', device)
        psnrs.append(metric_utils.calculate_psnr_batch(gt, pred, border=0))
        ssims.append(metric_utils.calculate_ssim_batch(gt, pred, border=0))
    psnr, ssim = float(np.array(psnrs).mean()), float(np.array(ssims).mean())
    fid = lpips = NOT_COMPUTED
    print('FID and LPIPS are not computed (-100): their networks (Inception, VGG) are not shipped with this project')
    print('-----------------------------------------')
    print('pred_root_path', pred_root_path)
    print('gt_root_path', gt_root_path)
    print('sample num', len(names))
    print('fid\tlpips\tpsnr\tssim')
    print(fid, '\t', lpips, '\t', psnr, '\t', ssim, '\t')
    print('-----------------------------------------')
    now = time.strftime("%Y_%m_%d %H.%M.%S\n", time.localtime())
    result_file = os.path.join(os.path.dirname(os.path.abspath(pred_root_path).rstrip(os.sep)), f'{now.strip()}_eval_result.txt')
    with open(result_file, "a", encoding="utf-8") as f:
        f.write(now + f'pred root path: {pred_root_path}\nGT root path: {gt_root_path}\nsample num: {len(names)}\n'
                'fid\tlpips\tpsnr\tssim\n' + f'{fid}\t{lpips}\t{psnr}\t{ssim}\t')
    return dict(fid=fid, lpips=lpips, psnr=psnr, ssim=ssim, sample_num=len(names), result_file=result_file)


def main(argv=None):
    p = argparse.ArgumentParser("run evaluation")
    p.add_argument("--pred_root_path", type=str, required=True, help="<...>/rendered_imgs of the results: <cls_id>/<shape>/albedo_%%03d.png")
    p.add_argument("--gt_root_path", type=str, required=True, help="<...>/rendered_imgs of the ground truth (color_%%03d.png or albedo_%%03d.png)")
    p.add_argument("--view_num", type=int, default=20)
    p.add_argument("--rendered_img_res", type=int, default=512)
    args = p.parse_args(argv)
    return eval(args.pred_root_path, args.gt_root_path, args.view_num, args.rendered_img_res)


if __name__ == '__main__':
    main()
