"""PSNR and SSIM of rendered views on the device (utils/metric_utils/psnr_ssmi.py:44-147), same names and argument order:
`calculate_psnr_batch(gt, pred, border=0, use_sk=True)` and `calculate_ssim_batch(...)` take two uint8 batches [N,H,W,C] on the
GPU and return the batch mean as a python float.  One kernel (csrc/metrics.hip) gives, per image, the exact integer sum of squared
differences and the float64 mean SSIM; PSNR = 10 log10(255^2 / (SSE / (H W C))) is formed on the host from the integer, which
equals both branches of the reference (`peak_signal_noise_ratio(data_range=255)` and `20 log10(255 / sqrt(mse))`), inf at SSE = 0.

use_sk=True  (the reference's default): skimage.metrics.structural_similarity(data_range=255, channel_axis=2) as published -- 7x7
             uniform window, sample covariance, 3-pixel border cropped.  Like the reference's skimage calls, it ignores `border`.
use_sk=False: psnr_ssmi.py:101-147 -- `border` pixels cropped first, 11x11 Gaussian window of sigma 1.5, "valid" region, population
             covariance.  (The reference averages three identical whole-array calls for 3-channel input: the mean over everything.)
An image smaller than the window is a ValueError.  skimage and cv2 are not dependencies."""
import math

import torch

from . import _lib
from ._lib import ptr, stream, check

WINDOW = {True: 7, False: 11}


def image_metrics(gt_imgs, pred_imgs, use_sk=True, want_ssim=True):
    """Per-image (sse [N] int64, ssim [N] float64 or None) of two uint8 [N,H,W,C] GPU batches (pdhip_image_metrics)."""
    if gt_imgs.shape != pred_imgs.shape:
        raise ValueError('Input images must have the same dimensions.')
    if gt_imgs.dim() != 4 or gt_imgs.dtype != torch.uint8 or pred_imgs.dtype != torch.uint8:
        raise ValueError(f'expected two uint8 batches [N,H,W,C], got {tuple(gt_imgs.shape)} {gt_imgs.dtype} / {pred_imgs.dtype}')
    N, H, W, C = gt_imgs.shape
    if N < 1 or not 1 <= C <= 4:
        raise ValueError(f'expected N >= 1 and 1 .. 4 channels, got N = {N}, C = {C}')
    win = WINDOW[bool(use_sk)]
    if want_ssim and (H < win or W < win):
        raise ValueError(f'a {H} x {W} image is smaller than the {win} x {win} SSIM window')
    L = _lib.lib()
    a, b = gt_imgs.contiguous(), pred_imgs.contiguous()
    dev = a.device
    sse = torch.empty((N,), dtype=torch.int64, device=dev)
    ssim = torch.empty((N,), dtype=torch.float64, device=dev) if want_ssim else None
    ws = torch.empty((max(1, L.pdhip_image_metrics_workspace_bytes(N, H, W)),), dtype=torch.uint8, device=dev)
    check(L.pdhip_image_metrics(ptr(a), ptr(b), N, H, W, C, 0 if use_sk else 1, ptr(sse), ptr(ssim, allow_none=True), ptr(ws), stream()),
          'pdhip_image_metrics')
    return sse, ssim


def _crop(x, border, use_sk):
    if border and not use_sk:
        h, w = x.shape[1:3]
        return x[:, border:h - border, border:w - border].contiguous()
    return x


def psnr_from_sse(sse, count):
    """10 log10(255^2 / (sse / count)) in float64, inf at sse = 0."""
    return [float('inf') if s == 0 else 10.0 * math.log10(255.0 ** 2 / (s / count)) for s in sse]


def calculate_psnr_batch(gt_imgs, pred_imgs, border=0, use_sk=True, return_per_image=False):
    """psnr_ssmi.py:44-71.  Returns the batch mean; return_per_image=True: (per-image PSNR [N] float64 tensor, sse [N] int64)."""
    gt_imgs, pred_imgs = _crop(gt_imgs, border, use_sk), _crop(pred_imgs, border, use_sk)
    sse, _ = image_metrics(gt_imgs, pred_imgs, use_sk, want_ssim=False)
    sse_host = sse.cpu()
    per = psnr_from_sse(sse_host.tolist(), gt_imgs.shape[1] * gt_imgs.shape[2] * gt_imgs.shape[3])
    if return_per_image:
        return torch.tensor(per, dtype=torch.float64), sse_host
    return sum(per) / len(per)


def calculate_ssim_batch(gt_imgs, pred_imgs, border=0, use_sk=True, return_per_image=False):
    """psnr_ssmi.py:76-99.  Returns the batch mean; return_per_image=True: (per-image SSIM [N] float64 tensor, sse [N] int64)."""
    gt_imgs, pred_imgs = _crop(gt_imgs, border, use_sk), _crop(pred_imgs, border, use_sk)
    sse, ssim = image_metrics(gt_imgs, pred_imgs, use_sk, want_ssim=True)
    ssim_host = ssim.cpu()
    if return_per_image:
        return ssim_host, sse.cpu()
    return float(ssim_host.sum() / ssim_host.numel())
