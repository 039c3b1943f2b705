"""Synthetic stand-in for the reference's TEST item, MessytableDataset(train=False, onReal=True)
(datasets/messytable.py:184-404) -- the dictionary test.py:69-311 consumes (see tools/test_rehearsal.py, its restatement).
Like SyntheticMessytableDataset, which it imports and whose geometry it renders (a smooth random depth field, textured
views with IR dots, the right view moved by the rounded disparity), it renders items on the device: same keys, shapes,
dtypes and value conventions as the reference's, with H x W the simulated size (540 x 960 there) and Hr x Wr = real_size
the size of the real captures (720 x 1280 there):

  img_sim_L / img_sim_R            [3,H,W]    float32   ImageNet-normalised grey images (messytable.py:278-280)
  img_disp_L / img_disp_R          [1,2H,2W]  float32   disparity at the 2x resolution of the depth maps
  img_depth_L / img_depth_R        [1,2H,2W]  float32   metres
                                              The depth field is quantised to whole millimetres as uint16 -- what the
                                              reference reads from its 16-bit PNGs, messytable.py:197-198; holes of the right
                                              view are 0 -- and the four maps are depth_to_labels of those two maps: the K25
                                              kernel, with the bits of messytable.py:208-213, 281-284.  depth_mm(idx) returns
                                              the two uint16 maps.
  img_depth_sim_realsense          [2H,2W]    float64   the left depth with sensor noise and zero holes (:192, 272-277)
  focal_length, baseline           [1,1,1]    float32   (:286-297), the float64 scalars of stereo_constants rounded
  intrinsic, intrinsic_l           [3,3]      float64   numpy, on the host, as the reference's pickle delivers them
  extrinsic, extrinsic_l           [4,4]      float64   numpy (:298-301); the right camera's is the attribute extrinsic_r
  prefix                           str
  img_real_L / img_real_R          [3,Hr,Wr]  float32   the real captures, normalised only (:334-335, 393-404): the scene
                                              rendered at Hr x Wr with sensor noise, quantised to uint8 levels, then
                                              augment_images (v / 255, mean, std)
  img_depth_real_realsense         [Hr,Wr]    float64   (:320, 343-348) noisy depth with zero holes
  robot_mask                       [2H,2W]    float64   (:351-359: resized to the depth maps' size) 0 outside the arm, 1
                                              inside, fractions on its edge as the reference's resized 8-bit mask has them
  img_label                        [1,2H,2W]  float32   (:321, 400; the size of robot_mask, :358) integer object labels:
                                              several objects 0 .. objects - 1 and the background, label obj_num - 1
                                              (configs/config.py:56: table and ground)
and, in addition to the reference's keys,
  img_real_L_levels / img_real_R_levels  [Hr,Wr]  uint8  the grey levels img_real_L / R were normalised from: what a loader
                                              that keeps the captures as bytes delivers (prepare_test_images takes either).
Every tensor lives on the device; the default collate of a DataLoader stacks the items as it stacks the reference's."""
import numpy as np
import torch

from activezero_amd.datasets.dataset_utils_gpu import augment_images, depth_to_labels, stereo_constants
from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset


class SyntheticMessytableTestDataset(torch.utils.data.Dataset):
    def __init__(self, length=8, height=540, width=960, real_size=(720, 1280), device="cuda:0", seed=0, max_disp=192,
                 objects=5, obj_num=18):
        # (real_size is handed to _views per call: the training dataset's 0.75 rule does not bind a test item)
        self.base = SyntheticMessytableDataset(length, height, width, onReal=True, device=device, seed=seed,
                                               max_disp=max_disp)
        self.length, self.h, self.w, self.device = int(length), int(height), int(width), self.base.device
        self.real_size = (int(real_size[0]), int(real_size[1]))
        self.objects, self.obj_num = int(objects), int(obj_num)
        if not 0 < self.objects < self.obj_num:
            raise RuntimeError(f"objects {objects} must lie in [1, obj_num - 1 = {self.obj_num - 1}]")
        # the rig's metadata; focal_length and baseline are what the reference's two lines make of it
        f, b = self.base.focal_length, self.base.baseline
        self.intrinsic_l = np.array([[2 * f, 0, self.w], [0, 2 * f, self.h], [0, 0, 1]], dtype=np.float64)
        self.intrinsic = self.intrinsic_l.copy()
        self.extrinsic_l, self.extrinsic, self.extrinsic_r = np.eye(4), np.eye(4), np.eye(4)
        self.extrinsic_r[0, 3] = -b
        self.focal_length, self.baseline = stereo_constants(self.extrinsic_l, self.extrinsic_r, self.intrinsic_l)

    def __len__(self):
        return self.length

    @staticmethod
    def _as_uint16(levels):
        """integer values 0..65535 held in int32 -> uint16, through the bit pattern of int16"""
        return (levels - 65536 * (levels >= 32768)).to(torch.int16).view(torch.uint16)

    def _sim_views(self, idx):
        """the simulated views and their geometry: left, right, left depth, right depth (metres, 2x resolution)"""
        left, right, _, _, _, depth2, _, depth_r2 = self.base._views(self.base._gen(idx, 1))
        return left, right, depth2, depth_r2

    def _millimetres(self, depth2, depth_r2):
        mm = self._as_uint16((1000.0 * torch.stack([depth2, depth_r2])).round().clamp(0, 65535).to(torch.int32))
        return mm[0], mm[1]

    def depth_mm(self, idx):
        """(left, right) [2H,2W] uint16: the millimetre depth maps item `idx` takes its labels from"""
        return self._millimetres(*self._sim_views(idx)[2:])

    def _holes(self, depth, g, sigma=0.002, share=0.1):
        """a RealSense-like reading of `depth`: noise of `sigma` metres, a `share` of the pixels lost (0), float64"""
        noisy = depth.double() + sigma * torch.randn(depth.shape, device=self.device, generator=g, dtype=torch.float64)
        lost = torch.rand(depth.shape, device=self.device, generator=g) < share
        return torch.where(lost, torch.zeros_like(noisy), noisy.clamp_min(0)).contiguous()

    def _label(self, g):
        """[2H,2W] float32: bands of a smooth field as objects 0 .. objects - 1, the background elsewhere"""
        hr, wr = 2 * self.h, 2 * self.w
        band = (self.base._smooth(g, hr, wr, 5) * self.objects).floor().clamp(0, self.objects - 1)
        ground = self.base._smooth(g, hr, wr, 3) < 0.4
        return torch.where(ground, torch.full_like(band, float(self.obj_num - 1)), band)

    def _robot_mask(self):
        """[2H,2W] float64: an arm in the upper left corner, 1 inside, 0.6 and 0.3 on the two pixels of its edge"""
        hr, wr = 2 * self.h, 2 * self.w
        ah, aw = max(hr // 4, 3), max(wr // 5, 3)
        m = torch.zeros(hr, wr, dtype=torch.float64, device=self.device)
        m[:ah, :aw] = 0.3
        m[:ah - 1, :aw - 1] = 0.6
        m[:ah - 2, :aw - 2] = 1.0
        return m

    def __getitem__(self, idx):
        left, right, depth2, depth_r2 = self._sim_views(idx)
        mm_l, mm_r = self._millimetres(depth2, depth_r2)
        disp_l, depth_l, disp_r, depth_r = depth_to_labels(mm_l, mm_r, self.focal_length, self.baseline)
        g = self.base._gen(idx, 4)
        # the same scene at the real camera's size (the same generator: the same depth field and texture), with sensor noise
        rl, rr, _, _, _, rdepth2, _, _ = self.base._views(self.base._gen(idx, 1), self.real_size)
        noise = lambda im: (im + 0.02 * torch.randn(im.shape, device=self.device, generator=g)).clamp(0, 1)  # noqa: E731
        levels = self.base._levels(torch.stack([noise(rl), noise(rr)]))
        real = augment_images(levels)
        one = lambda v: torch.full((1, 1, 1), float(v), dtype=torch.float32, device=self.device)  # noqa: E731
        return {
            "img_sim_L": self.base._normalise(left), "img_sim_R": self.base._normalise(right),
            "img_disp_L": disp_l, "img_depth_L": depth_l, "img_disp_R": disp_r, "img_depth_R": depth_r,
            "img_depth_sim_realsense": self._holes(depth2, g),
            "focal_length": one(self.focal_length), "baseline": one(self.baseline),
            "intrinsic": self.intrinsic, "intrinsic_l": self.intrinsic_l,
            "extrinsic": self.extrinsic, "extrinsic_l": self.extrinsic_l,
            "prefix": f"synthetic-test-{idx:05d}",
            "img_real_L": real[0].contiguous(), "img_real_R": real[1].contiguous(),
            "img_real_L_levels": levels[0].contiguous(), "img_real_R_levels": levels[1].contiguous(),
            "img_depth_real_realsense": self._holes(rdepth2[::2, ::2], g),
            "robot_mask": self._robot_mask(),
            "img_label": self._label(g)[None].contiguous(),
        }
