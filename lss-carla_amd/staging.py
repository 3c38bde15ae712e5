"""A SimBEV batch into the static tensors a captured step reads (train_simbev.py:229-240's ``.to(device)``).

A captured graph (train_step.TrainStep / EvalStep) reads fixed addresses: the images, the rig, the
labels, the host-inverted rig matrices (ops.HostInverses) and, for a partial batch, how many samples
are valid. ``BatchStager`` owns those tensors and fills them from the raw batches of
``simbev.compile_data``'s DataLoader (``DeviceLoader.loader``), one batch ahead of the step:

  stage(raw)   on the staging stream: H2D copies of the uint8 images / BEV and of the rig, then
               ``lss_simbev_images`` and ``lss_simbev_vehicle_mask`` (``lss_simbev_class_masks`` with
               ``label_groups``; ``lss_simbev_class_masks_warp`` with ``bev_aug``: the batch's label index
               matrices, uploaded on the same stream; with ``valid_mask``, ``lss_simbev_valid_mask`` into
               the slot's mask; with ``photo``, ``lss_simbev_images_photo`` in ``lss_simbev_images``' place, on
               the batch's photo records uploaded on the same stream) straight into the next of two slots;
               an event marks the slot ready. Batch k+1 is staged while step k runs.
  commit()     on the current stream: wait for the oldest staged slot's event, copy slot -> static tensors
               (device to device), ``HostInverses.update`` with the slot's host post_rots / intrins, set
               ``n_valid``; an event marks the slot consumed (the staging stream waits for it before it
               writes the slot again).

Stream rules. The staging stream runs copies and the simbev kernels only -- no plan, batch-norm or
depthwise kernel: their persistent workspaces (norm._sync, ops._PlanWorkspace) belong to one stream.
What ``stage`` allocates (the kernels' parameter block, a table concatenation) and the host batch its
copies read stay referenced until the slot's event has completed. Neither method synchronises the
host, except for the wait HostInverses does on a pinned buffer two updates old. A batch of b < B samples
fills samples 0..b-1; the rest of the static tensors keep their previous contents and ``n_valid = b``.
"""
from __future__ import annotations

from collections import deque
from typing import List, Sequence

import torch

from . import ops, simbev


class _Slot:
    def __init__(self, B, N, fH, fW, src_hw, K, X, Y, dev, exclusive=False):
        H, W = int(src_hw[0]), int(src_hw[1])
        self.u8 = torch.empty(B * N, H, W, 3, device=dev, dtype=torch.uint8)
        self.bev_u8 = None  # (B, classes, X, Y): sized by the first batch
        self.imgs = torch.zeros(B, N, 3, fH, fW, device=dev, dtype=torch.float32)
        self.rots = torch.zeros(B, N, 3, 3, device=dev)
        self.trans = torch.zeros(B, N, 3, device=dev)
        self.intrins = torch.zeros(B, N, 3, 3, device=dev)
        self.post_rots = torch.zeros(B, N, 3, 3, device=dev)
        self.post_trans = torch.zeros(B, N, 3, device=dev)
        if exclusive:  # the (B, X, Y) uint8 exclusive class map of the K groups
            self.binimgs = torch.zeros(B, X, Y, device=dev, dtype=torch.uint8)
        else:
            self.binimgs = torch.zeros(B, K, X, Y, device=dev, dtype=torch.float32)
        self.valid = None  # (B, X, Y) uint8, all ones, when the stager keeps a valid-cell mask
        self.host_post_rots = None
        self.host_intrins = None
        self.b = 0
        self.ready = None     # recorded on the staging stream after the slot is filled
        self.consumed = None  # recorded on the consumer's stream after commit's copies
        self.keep: list = []


class BatchStager:
    RIG = ("rots", "trans", "intrins", "post_rots", "post_trans")

    def __init__(self, final_dim: Sequence[int], B: int, N: int, src_hw: Sequence[int], grid: dict, device,
                 label_groups=None, bev_aug=False, valid_mask=None, fov_z=(0.0,), dbound=None, exclusive=False,
                 photo=False):
        """label_groups: K lists of BEV channels, one label channel each (simbev.class_masks): ``binimgs`` and
        both slots are (B, K, X, Y); None: the reference's vehicle mask, K = 1. bev_aug: the raw batches come from a
        conf with the BEV-space augmentation (simbev.bev_aug_enabled): the element before the BEV maps is the
        (b, 2, 3) label index matrices, which warp the labels; the rig arrives composed.
        valid_mask: None, "grid" or "fov" (simbev.valid_mask_mode): the stager then keeps ``valid``, the (B, X, Y) uint8
        valid-cell mask of the committed batch (all ones before the first), filled on the staging stream by
        ``lss_simbev_valid_mask`` from the batch's host rig (camera blocks built in float64, uploaded pinned on that
        stream and held until the slot's event) at the heights fov_z; dbound overrides the grid's frustum bounds.
        Training and validation batches are masked alike; without index matrices every cell is in the grid. With
        "fov" the mask comes from the cameras the batch actually holds: a stager of N < 6 cameras (training on a camera
        subset) marks a cell only a dropped camera would see invalid in that sample. ``cam_alive`` (an attribute, None
        or an (N,) / (B, N) host mask) further blanks dead cameras' blocks (simbev.fov_cameras(alive=)).
        exclusive: ``binimgs`` and both slots are the (B, X, Y) uint8 exclusive class map of the 1..7 label_groups
        (0 the background, k + 1 group k, a later group wins), written by ``lss_simbev_class_index`` on the staging
        stream in ``lss_simbev_class_masks``' place; nothing else differs.
        photo: the raw batches come from a conf with the photometric augmentation (simbev.photo_enabled): the element
        before the label index matrices (before the BEV maps without bev_aug) is the (b, N, 16) photo records, which
        the image kernel applies on the staging stream (simbev.augment_images, photo=); slots, events and partial
        batches are as without it, and only ``imgs`` differs."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("BatchStager: the static tensors live on the MI355X (no CPU fallback)")
        self.device, self.B, self.N = dev, int(B), int(N)
        self.final_dim = (int(final_dim[0]), int(final_dim[1]))
        fH, fW = self.final_dim
        X, Y, _ = ops.GridSpec.from_conf(grid).nx
        self.imgs = torch.zeros(B, N, 3, fH, fW, device=dev, dtype=torch.float32)
        eye = torch.eye(3, device=dev).expand(B, N, 3, 3)
        self.rots, self.intrins, self.post_rots = (eye.clone() for _ in range(3))
        self.trans = torch.zeros(B, N, 3, device=dev)
        self.post_trans = torch.zeros(B, N, 3, device=dev)
        if label_groups is not None:
            simbev.group_bits(label_groups)
        self.label_groups = None if label_groups is None else [list(g) for g in label_groups]
        self.bev_aug = bool(bev_aug)
        self.photo = bool(photo)
        K = 1 if label_groups is None else len(self.label_groups)
        self.exclusive = bool(exclusive)
        if self.exclusive:
            if label_groups is None:
                raise ValueError("BatchStager: exclusive classes need label_groups")
            simbev.exclusive_bits(label_groups)
            self.binimgs = torch.zeros(B, X, Y, device=dev, dtype=torch.uint8)
        else:
            self.binimgs = torch.zeros(B, K, X, Y, device=dev, dtype=torch.float32)
        if valid_mask is not None and valid_mask not in simbev.VALID_MASK_MODES:
            raise ValueError(f"BatchStager: valid_mask {valid_mask!r}: None, grid or fov")
        self.valid_mask = valid_mask
        self.fov_z = simbev.fov_heights({"fov_z": fov_z})
        self.grid = dict(grid) if dbound is None else {**grid, "dbound": list(dbound)}
        self.valid = None if valid_mask is None else torch.ones(B, X, Y, device=dev, dtype=torch.uint8)
        self.n_valid = torch.full((1,), B, device=dev, dtype=torch.int32)
        self.cam_alive = None  # host mask of the cameras "fov" may count: (N,) or (B, N); None: every camera
        self.hinv = ops.HostInverses(B * N, dev)
        # the host rig HostInverses inverts: samples past a partial batch keep their previous matrices
        self._host_post_rots = torch.eye(3).repeat(B, N, 1, 1)
        self._host_intrins = torch.eye(3).repeat(B, N, 1, 1)
        self.stream = torch.cuda.Stream(dev)
        if self.exclusive:
            self._slots = [_Slot(B, N, fH, fW, src_hw, K, X, Y, dev, exclusive=True) for _ in range(2)]
        else:
            self._slots = [_Slot(B, N, fH, fW, src_hw, K, X, Y, dev) for _ in range(2)]
        if valid_mask is not None:
            for slot in self._slots:
                slot.valid = torch.ones(B, X, Y, device=dev, dtype=torch.uint8)
        self._next = 0
        self._staged: deque = deque()   # slots staged and not yet committed, oldest first
        self._retired: List[tuple] = []  # (event, tensors) of reused slots whose event had not completed

    @property
    def inputs(self):
        """The model's six static inputs, in forward's order."""
        return (self.imgs, self.rots, self.trans, self.intrins, self.post_rots, self.post_trans)

    def pending(self) -> int:
        return len(self._staged)

    def stage(self, raw_batch) -> None:
        """Fill the next slot from a collated raw batch (simbev.SegmentationData's samples)."""
        if len(self._staged) >= len(self._slots):
            raise RuntimeError("BatchStager.stage: both slots hold uncommitted batches (commit() first)")
        imgs_u8, rots, trans, intrins, post_rots, post_trans, aug, rot = raw_batch[:8]
        bev = raw_batch[-1]
        index_mats = raw_batch[-2] if self.bev_aug else None
        records = raw_batch[-3 if self.bev_aug else -2] if self.photo else None
        b, N = int(imgs_u8.shape[0]), int(imgs_u8.shape[1])
        slot = self._slots[self._next]
        if not 0 < b <= self.B or N != self.N or tuple(imgs_u8.shape[2:]) != tuple(slot.u8.shape[1:]):
            raise RuntimeError(f"BatchStager.stage: batch of images {tuple(imgs_u8.shape)} does not fit "
                               f"B={self.B}, N={self.N}, source {tuple(slot.u8.shape[1:3])}")
        if bev.dtype == torch.bool:
            bev = bev.view(torch.uint8)
        if bev.dtype != torch.uint8 or bev.dim() != 4 or tuple(bev.shape[2:]) != tuple(slot.binimgs.shape[-2:]):
            raise RuntimeError(f"BatchStager.stage: BEV maps {bev.dtype} {tuple(bev.shape)} against labels "
                               f"{tuple(slot.binimgs.shape)}")
        if index_mats is not None and (index_mats.dtype != torch.float32 or tuple(index_mats.shape) != (b, 2, 3)):
            raise RuntimeError(f"BatchStager.stage: label index matrices {index_mats.dtype} "
                               f"{tuple(index_mats.shape)} for a batch of {b} (a raw batch without the BEV-space "
                               "augmentation?)")
        if records is not None and (not torch.is_tensor(records) or records.dtype != torch.float32
                                    or tuple(records.shape) != (b, N, simbev.PHOTO_WORDS)):
            raise RuntimeError(f"BatchStager.stage: photo records {getattr(records, 'dtype', None)} "
                               f"{tuple(getattr(records, 'shape', ()))} for a batch of {b} x {N} images (a raw batch "
                               "without the photometric augmentation?)")
        self._next ^= 1
        self._retire(slot)
        augs = []
        for i in range(b):
            a = aug[i].tolist()
            rec = {"resize_dims": (a[0], a[1]), "crop": tuple(a[2:6]), "flip": bool(a[6]), "rotate": float(rot[i])}
            augs.extend([rec] * N)
        keep = [raw_batch]  # the copies below read the batch's host memory
        cams = None
        if self.valid_mask == "fov":  # the camera blocks of the batch's (composed) rig: host float64, rounded once
            alive = self.cam_alive
            if alive is not None and torch.as_tensor(alive).dim() == 2:
                alive = torch.as_tensor(alive)[:b]
            cams = simbev.fov_cameras(rots, trans, intrins, post_rots, alive=alive)
        st = self.stream
        if slot.consumed is not None:
            st.wait_event(slot.consumed)  # commit's copies out of this slot come first
        with torch.cuda.stream(st):
            if slot.bev_u8 is None or slot.bev_u8.shape[1] != bev.shape[1]:
                slot.bev_u8 = torch.empty(self.B, *bev.shape[1:], device=self.device, dtype=torch.uint8)
            slot.u8[:b * N].copy_(imgs_u8.reshape(b * N, *imgs_u8.shape[2:]), non_blocking=True)
            slot.bev_u8[:b].copy_(bev, non_blocking=True)
            for name, t in zip(self.RIG, (rots, trans, intrins, post_rots, post_trans)):
                getattr(slot, name)[:b].copy_(t, non_blocking=True)
            if records is None:
                simbev.augment_images(slot.u8[:b * N], augs, self.final_dim, out=slot.imgs[:b], keep=keep)
            else:
                simbev.augment_images(slot.u8[:b * N], augs, self.final_dim, out=slot.imgs[:b], keep=keep,
                                      photo=records.reshape(b * N, simbev.PHOTO_WORDS))
            if self.exclusive:
                simbev.class_index(slot.bev_u8[:b], self.label_groups, out=slot.binimgs[:b], index_mats=index_mats,
                                   keep=keep)
            else:
                simbev.class_masks(slot.bev_u8[:b], self.label_groups, out=slot.binimgs[:b], index_mats=index_mats,
                                   keep=keep)
            if self.valid_mask is not None:
                simbev.valid_mask(cams, post_trans if cams is not None else None, self.grid, self.final_dim,
                                  self.fov_z, index_mats=index_mats, mode=self.valid_mask, out=slot.valid[:b],
                                  keep=keep)
            slot.ready = torch.cuda.Event()
            slot.ready.record(st)
        slot.host_post_rots, slot.host_intrins, slot.b, slot.keep = post_rots, intrins, b, keep
        self._staged.append(slot)

    def commit(self) -> int:
        """The oldest staged batch into the static tensors, on the current stream; returns its size."""
        if not self._staged:
            raise RuntimeError("BatchStager.commit: nothing staged")
        slot = self._staged.popleft()
        b = slot.b
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(slot.ready)
        for name in ("imgs", "binimgs") + self.RIG:
            getattr(self, name)[:b].copy_(getattr(slot, name)[:b], non_blocking=True)
        if self.valid is not None:
            self.valid[:b].copy_(slot.valid[:b], non_blocking=True)
        self._host_post_rots[:b].copy_(slot.host_post_rots)
        self._host_intrins[:b].copy_(slot.host_intrins)
        self.hinv.update(self._host_post_rots, self._host_intrins)
        self.n_valid.fill_(b)
        slot.consumed = torch.cuda.Event()
        slot.consumed.record(cur)
        return b

    def _retire(self, slot: _Slot) -> None:
        """Drop the tensors a slot kept for its last batch once its event has completed (else later)."""
        self._retired = [(e, k) for e, k in self._retired if not e.query()]
        if slot.keep and slot.ready is not None and not slot.ready.query():
            self._retired.append((slot.ready, slot.keep))
        slot.keep = []
