"""PSNR / SSIM on the GPU (csrc/metrics.hip, pointdreamer_amd/metric_utils.py, the run_evaluation CLI) against the numpy float64
references of tests/render_common.py: the integer SSE exactly, SSIM within 1e-9 absolute under both definitions (the cancellation
in E[x^2] - mu^2 is at most 121 * 65025 * 2^-52 ~ 1.7e-9 before the division by C2 ~ 58.5, ~3e-11 after it), bit-equal repeats,
refusal of undersized images, batch means, and an evaluation of a directory against itself."""
import math
import os

import numpy as np
import PIL.Image
import pytest
import torch

import render_common as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [(7, 7), (11, 11), (12, 17), (64, 64), (70, 45)]          # one window each; tile borders (32 x 16 output tiles) crossed
N = 3


def batches(H, W, C, seed):
    """name -> (a, b) uint8 [N,H,W,C]: random pairs, an image against itself, constants, an image against itself plus 1."""
    rng = np.random.default_rng(seed)
    r = lambda hi=256: rng.integers(0, hi, size=(N, H, W, C), dtype=np.uint8)
    a = r()
    low = r(255)
    const_a = np.broadcast_to(np.array([10, 200, 128], np.uint8)[:, None, None, None], (N, H, W, C)).copy()
    const_b = np.broadcast_to(np.array([200, 37, 128], np.uint8)[:, None, None, None], (N, H, W, C)).copy()
    return {'random': (a, r()), 'self': (a, a.copy()), 'constant': (const_a, const_b), 'plus_one': (low, low + 1)}


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_sse_exact_and_ssim_within_1e9_of_the_reference(H, W, C):
    from pointdreamer_amd import metric_utils as mu
    for name, (a, b) in batches(H, W, C, seed=H * 100 + W + C).items():
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        for use_sk in (True, False):
            if H < mu.WINDOW[use_sk] or W < mu.WINDOW[use_sk]:
                with pytest.raises(ValueError):
                    mu.calculate_ssim_batch(ta, tb, use_sk=use_sk)
                continue
            ssim, sse = mu.calculate_ssim_batch(ta, tb, use_sk=use_sk, return_per_image=True)
            ssim2, sse2 = mu.calculate_ssim_batch(ta, tb, use_sk=use_sk, return_per_image=True)
            assert ssim.dtype == torch.float64 and sse.dtype == torch.int64
            assert torch.equal(ssim, ssim2) and torch.equal(sse, sse2)                       # two runs: equal bits
            for n in range(N):
                want = rc.ssim_ref(a[n], b[n], use_sk)
                p_want, sse_want = rc.psnr_ref(a[n], b[n])
                print(f'{H}x{W}x{C} {name} use_sk={use_sk} image {n}: ssim error {abs(float(ssim[n]) - want):.2e}')
                assert int(sse[n]) == sse_want, (name, n)
                assert abs(float(ssim[n]) - want) <= 1e-9, (name, use_sk, n, float(ssim[n]), want)
            if name == 'self':
                assert torch.all((ssim - 1.0).abs() <= 1e-12) and torch.all(sse == 0)
            if name == 'plus_one':
                assert torch.all(sse == H * W * C)
            if name == 'constant':
                for n, (x, y) in enumerate(((10, 200), (200, 37), (128, 128))):
                    assert abs(float(ssim[n]) - (2.0 * x * y + rc.C1) / (x * x + y * y + rc.C1)) <= 1e-12
        psnr, sse = mu.calculate_psnr_batch(ta, tb, return_per_image=True)
        for n in range(N):
            p_want, sse_want = rc.psnr_ref(a[n], b[n])
            assert int(sse[n]) == sse_want
            assert float(psnr[n]) == p_want if math.isinf(p_want) else abs(float(psnr[n]) - p_want) <= 1e-12 * p_want


def test_batch_functions_return_the_batch_mean_and_crop_the_border():
    from pointdreamer_amd import metric_utils as mu
    a, b = batches(40, 52, 3, seed=9)['random']
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for use_sk in (True, False):
        per, _ = mu.calculate_ssim_batch(ta, tb, use_sk=use_sk, return_per_image=True)
        assert abs(mu.calculate_ssim_batch(ta, tb, use_sk=use_sk) - float(per.mean())) <= 1e-15
        assert abs(mu.calculate_ssim_batch(ta, tb, use_sk=use_sk) - np.mean([rc.ssim_ref(a[n], b[n], use_sk) for n in range(N)])) <= 1e-9
        pp, _ = mu.calculate_psnr_batch(ta, tb, use_sk=use_sk, return_per_image=True)
        assert abs(mu.calculate_psnr_batch(ta, tb, use_sk=use_sk) - float(pp.mean())) <= 1e-12
    # the reference's own branch (use_sk=False) crops `border` pixels first; its skimage branch ignores the argument
    want = np.mean([rc.ssim_ref(a[n, 4:-4, 4:-4], b[n, 4:-4, 4:-4], False) for n in range(N)])
    assert abs(mu.calculate_ssim_batch(ta, tb, border=4, use_sk=False) - want) <= 1e-9
    assert mu.calculate_ssim_batch(ta, tb, border=4, use_sk=True) == mu.calculate_ssim_batch(ta, tb, use_sk=True)
    want = np.mean([rc.psnr_ref(a[n, 4:-4, 4:-4], b[n, 4:-4, 4:-4])[0] for n in range(N)])
    assert abs(mu.calculate_psnr_batch(ta, tb, border=4, use_sk=False) - want) <= 1e-12 * want
    assert mu.calculate_psnr_batch(ta, ta) == float('inf')


def test_c_abi_refuses_an_undersized_image_on_the_device():
    from pointdreamer_amd import _lib
    from pointdreamer_amd._lib import ptr
    L = _lib.lib()
    a = torch.zeros((1, 6, 9, 3), dtype=torch.uint8, device=DEV)
    out = torch.zeros((1,), dtype=torch.float64, device=DEV)
    ws = torch.zeros((4096,), dtype=torch.uint8, device=DEV)
    assert L.pdhip_image_metrics(ptr(a), ptr(a), 1, 6, 9, 3, 0, None, ptr(out), ptr(ws), _lib.stream()) == -1
    assert b'smaller than the 7 x 7' in L.pdhip_last_error()
    sse = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    assert L.pdhip_image_metrics(ptr(a), ptr(a), 1, 6, 9, 3, 0, ptr(sse), None, ptr(ws), _lib.stream()) == 0        # PSNR alone needs no window
    assert int(sse[0]) == 0


def test_run_evaluation_of_a_directory_against_itself(tmp_path):
    from pointdreamer_amd import run_evaluation
    rng = np.random.default_rng(4)
    pred = tmp_path / 'run' / 'rendered_imgs'
    for shape in ('s0', 's1'):
        d = pred / 'cls' / shape
        os.makedirs(d)
        for v in range(2):
            img = rng.integers(0, 256, size=(32, 32, 4), dtype=np.uint8)
            img[..., 3] = np.where(rng.random((32, 32)) < 0.3, 0, 255)
            PIL.Image.fromarray(img, 'RGBA').save(d / f'albedo_{v + 1:03d}.png')
    got = run_evaluation.imread(str(pred / 'cls' / 's0' / 'albedo_001.png'))
    raw = np.array(PIL.Image.open(pred / 'cls' / 's0' / 'albedo_001.png'))
    assert got.shape == (32, 32, 3) and np.all(got[raw[..., 3] == 0] == (0, 255, 0)) and np.array_equal(got[raw[..., 3] > 0], raw[..., :3][raw[..., 3] > 0])
    res = run_evaluation.main(['--pred_root_path', str(pred), '--gt_root_path', str(pred), '--view_num', '2', '--rendered_img_res', '32'])
    assert res['psnr'] == float('inf') and abs(res['ssim'] - 1.0) <= 1e-12 and res['fid'] == -100 and res['lpips'] == -100
    assert res['sample_num'] == 2 and os.path.dirname(res['result_file']) == str(tmp_path / 'run')
    lines = open(res['result_file']).read().split('\n')
    assert lines[-2] == 'fid\tlpips\tpsnr\tssim' and lines[-1] == '-100\t-100\tinf\t1.0\t'
    res16 = run_evaluation.eval(str(pred), str(pred), view_num=2, rendered_img_res=16)                                # the resize path
    assert res16['psnr'] == float('inf')
