"""Synthetic stand-in for the reference's MessytableDataset (datasets/messytable.py:184-306 sim item,
:308-404 real item) -- SURVEY.md 8f-4.  The private MessyTable data cannot travel, so this dataset RENDERS
items of the same dictionary shape on the device: same keys, shapes, dtypes and value conventions, so that
the loop of train.py:220-432 (see tools/train_rehearsal.py, its restatement for the keys this path consumes)
runs end to end without the dataset:

  img_sim_L / img_sim_R            [3,H,W]   ImageNet-normalised grey images (dataset_utils.py:76-81)
  img_sim_L_reproj / _R_reproj     [1,H,W]   binary IR pattern, extracted ON THE GPU from the (IR, no-IR)
                                             image pair with get_smoothed_ir_pattern2 (dataset_utils.py:33-46)
  img_disp_L / img_disp_R          [1,2H,2W] disparity at the 2x resolution of the depth maps (messytable.py:252-261)
  img_depth_L / img_depth_R        [1,2H,2W] metres;  focal_length, baseline [1,1,1];  prefix (str)
  (onReal) img_real_L / img_real_R [3,H,W],  img_real_L_reproj / img_real_R_reproj [1,H,W]
  (onReal, temporal=True) the two real patterns are the reference's TEMPORAL patterns (tools/temporal_ir.py:91-114, read
                                             back by messytable.py:406-426): per view a stack of 7 projector exposures
                                             [7,H,W] uint8 is rendered -- exposure k = texture + (k/6) dot gain + sensor
                                             noise, quantised to 0..255 -- and passed through get_temporal_ir_pattern
  (augment=True) img_sim_L / img_sim_R go through the reference's data_augmentation with both of its switches on
                                             (messytable.py:264-270: one drawn sigma, brightness and contrast for both
                                             views; configs/config.py:104-113), on the device; the real images keep the
                                             normalisation only (messytable.py:402-404)
  (real_size=(Hr, Wr))                       the real views are rendered at Hr x Wr, quantised to uint8 levels
                                             (round(255 x)) and brought to H x W = (int(0.75 Hr), int(0.75 Wr)) by
                                             resize_bilinear, PIL's 8-bit BILINEAR resize on the device, as
                                             messytable.py:324-341 takes its 720 x 1280 captures to 540 x 960: img_real_L / R
                                             are augment_images of the resized levels (normalisation only), the patterns
                                             come from the resized float images; with temporal=True the exposure stack is
                                             rendered at Hr x Wr, get_temporal_ir_pattern runs there and its 0 / 1 pattern
                                             is resized as levels 0 / 255 to float32, as messytable.py:410-420 resizes
                                             the stored pattern -- values in [0,1], no longer binary.  (The reference's
                                             stored pattern is a PNG that tools/temporal_ir.py wrote through matplotlib's
                                             colour map and that the loader converts from RGB back to grey before the
                                             resize; that round trip is not reproduced.)  Keys, shapes and dtypes are
                                             those of the default, which renders the real views at H x W directly.

Geometry: a smooth random depth field -> disparity = focal * baseline / depth; the right view is the left one
moved by the (integer-rounded) disparity with the scatter warp K1, so disparity, images and patterns are
mutually consistent and the losses have signal."""
import torch
import torch.nn.functional as F

from activezero_amd.datasets.dataset_utils_gpu import (augment_images, data_augmentation, get_smoothed_ir_pattern2,
                                                       get_temporal_ir_pattern, resize_bilinear)
from activezero_amd.utils.warp_ops import apply_disparity_cu

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


class SyntheticMessytableDataset(torch.utils.data.Dataset):
    def __init__(self, length=64, height=256, width=512, onReal=True, device="cuda:0", seed=0, max_disp=192,
                 temporal=False, augment=False, real_size=None):
        self.temporal, self.augment = bool(temporal), bool(augment)
        self.length, self.h, self.w, self.onReal = int(length), int(height), int(width), bool(onReal)
        self.real_size = None if real_size is None else (int(real_size[0]), int(real_size[1]))
        if self.real_size is not None and (int(self.real_size[0] * 0.75), int(self.real_size[1] * 0.75)) != (self.h, self.w):
            raise RuntimeError(f"real_size {self.real_size} scaled by 0.75 (messytable.py:324-341) is not "
                               f"(height, width) = {(self.h, self.w)}")
        self.device, self.seed, self.max_disp = torch.device(device), int(seed), int(max_disp)
        self.focal_length, self.baseline = 446.31, 0.055  # the order of the MessyTable rig (metres, half-res pixels)

    def __len__(self):
        return self.length

    def _gen(self, idx, salt):
        return torch.Generator(device=self.device).manual_seed(self.seed * 1000003 + idx * 7 + salt)

    def _smooth(self, g, h, w, cells):
        low = torch.rand(1, 1, cells, 2 * cells, device=self.device, generator=g)
        return F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1)[0, 0]

    def _views(self, g, size=None):
        """(left, right) grey images with IR dots, their no-IR versions, left/right disparity at 2x resolution; at
        `size` = (h, w) instead of the item's"""
        h, w = (self.h, self.w) if size is None else size
        depth2 = 0.45 + 1.1 * self._smooth(g, 2 * h, 2 * w, 6)             # metres, 2x resolution
        disp2 = self.focal_length * self.baseline / depth2                 # half-res pixels (messytable.py:205-213)
        disp = F.avg_pool2d(disp2[None, None], 2)[0, 0]
        tex = 0.25 + 0.5 * self._smooth(g, h, w, 24)
        dots = (torch.rand(h, w, device=self.device, generator=g) < 0.06).float()
        left_no_ir, left = tex, (tex + 0.35 * dots).clamp(0, 1)
        shift = (-disp.round()).int()[None, None].contiguous()             # left -> right: x - d
        warp = lambda im: apply_disparity_cu(im[None, None].contiguous(), shift)[0, 0]
        right, right_no_ir = warp(left), warp(left_no_ir)
        disp_r2 = F.interpolate(warp(disp)[None, None], scale_factor=2, mode="nearest")[0, 0]
        depth_r2 = torch.where(disp_r2 > 0, self.focal_length * self.baseline / disp_r2.clamp_min(1e-6),
                               torch.zeros_like(disp_r2))
        return left, right, left_no_ir, right_no_ir, disp2, depth2, disp_r2, depth_r2

    def _normalise(self, grey):
        rgb = grey[None].expand(3, -1, -1)
        mean = torch.tensor(_MEAN, device=self.device).view(3, 1, 1)
        std = torch.tensor(_STD, device=self.device).view(3, 1, 1)
        return ((rgb - mean) / std).contiguous()

    def _real_views(self, idx):
        """the real item's generator, noisy (left, right), their no-IR versions and the noise-free lit pair [2,H,W]; at
        real_size when one is set"""
        g = self._gen(idx, 2)
        rl, rr, rl0, rr0, *_ = self._views(g, self.real_size)
        lit = torch.stack([rl, rr])
        noise = lambda im: (im + 0.02 * torch.randn(im.shape, device=self.device, generator=g)).clamp(0, 1)
        return g, noise(rl), noise(rr), rl0, rr0, lit

    def _exposures(self, g, lit, unlit, frames=7, sigma=1.5):
        """[2,frames,H,W] uint8: both views at projector power k / (frames - 1), sensor noise of `sigma` grey levels"""
        power = torch.linspace(0, 1, frames, device=self.device).view(1, frames, 1, 1)
        level = 255.0 * (unlit[:, None] + power * (lit - unlit)[:, None])
        level = level + sigma * torch.randn(level.shape, device=self.device, generator=g)
        return level.round().clamp(0, 255).to(torch.uint8)

    def _temporal_stack(self, idx):
        """the exposure stack item `idx` takes its real patterns from (temporal=True); for tests"""
        g, _, _, rl0, rr0, lit = self._real_views(idx)
        return self._exposures(g, lit, torch.stack([rl0, rr0]))

    @staticmethod
    def _levels(x):
        """[0,1] images as uint8 grey levels, what a sensor stores"""
        return (255.0 * x).round().clamp(0, 255).to(torch.uint8)

    def _real_levels(self, idx):
        """[4,Hr,Wr] uint8: the levels item `idx` resizes (real_size set) -- left, right and their no-IR versions; for tests"""
        _, rl, rr, rl0, rr0, _ = self._real_views(idx)
        return self._levels(torch.stack([rl, rr, rl0, rr0]))

    def _real_resized(self, g, rl, rr, rl0, rr0, lit):
        """the real entries of an item whose views were rendered at real_size: everything passes through resize_bilinear"""
        size = (self.h, self.w)
        levels = self._levels(torch.stack([rl, rr, rl0, rr0]))
        real = augment_images(resize_bilinear(levels[:2], size))
        if self.temporal:
            native = get_temporal_ir_pattern(self._exposures(g, lit, torch.stack([rl0, rr0])))
            rpat = resize_bilinear((255.0 * native).to(torch.uint8), size, dtype=torch.float32)
        else:
            grey = resize_bilinear(levels, size, dtype=torch.float32)
            rpat = get_smoothed_ir_pattern2(grey[:2], grey[2:])
        return {"img_real_L": real[0].contiguous(), "img_real_R": real[1].contiguous(),
                "img_real_L_reproj": rpat[0:1].contiguous(), "img_real_R_reproj": rpat[1:2].contiguous()}

    def _augmentation(self, idx):
        return data_augmentation(True, True, generator=self._gen(idx, 3))

    def augmentation_params(self, idx):
        """what item `idx` is augmented with (augment=True): sigma, brightness, contrast (one value each, shared by the two
        views) and contrast_first [2] (left, right); for tests"""
        aug = self._augmentation(idx)
        return {"sigma": aug.sigma, "brightness": aug.brightness, "contrast": aug.contrast,
                "contrast_first": aug.draw_order(2)}

    def __getitem__(self, idx):
        g = self._gen(idx, 1)
        left, right, left0, right0, disp2, depth2, disp_r2, depth_r2 = self._views(g)
        pat = get_smoothed_ir_pattern2(torch.stack([left, right]), torch.stack([left0, right0]))
        item = {
            "img_sim_L": self._normalise(left), "img_sim_R": self._normalise(right),
            "img_sim_L_reproj": pat[0:1].contiguous(), "img_sim_R_reproj": pat[1:2].contiguous(),
            "img_disp_L": disp2[None].contiguous(), "img_depth_L": depth2[None].contiguous(),
            "img_disp_R": disp_r2[None].contiguous(), "img_depth_R": depth_r2[None].contiguous(),
            "prefix": f"synthetic-{idx:05d}",
            "focal_length": torch.full((1, 1, 1), self.focal_length, device=self.device),
            "baseline": torch.full((1, 1, 1), self.baseline, device=self.device),
        }
        if self.augment:
            pair = self._augmentation(idx)(torch.stack([left, right])[None])[0]
            item["img_sim_L"], item["img_sim_R"] = pair[0].contiguous(), pair[1].contiguous()
        if self.onReal:
            g, rl, rr, rl0, rr0, lit = self._real_views(idx)
            if self.real_size is not None:
                item.update(self._real_resized(g, rl, rr, rl0, rr0, lit))
                return item
            if self.temporal:
                rpat = get_temporal_ir_pattern(self._exposures(g, lit, torch.stack([rl0, rr0])))
            else:
                rpat = get_smoothed_ir_pattern2(torch.stack([rl, rr]), torch.stack([rl0, rr0]))
            item.update({"img_real_L": self._normalise(rl), "img_real_R": self._normalise(rr),
                         "img_real_L_reproj": rpat[0:1].contiguous(), "img_real_R_reproj": rpat[1:2].contiguous()})
        return item
