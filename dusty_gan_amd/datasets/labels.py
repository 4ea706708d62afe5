"""Semantic labels on the range image: the SemanticKITTI branch of the reference's process_kitti.py
(:120-131) - every scan's `.label` file projected onto the range image like the points, written as a palette PNG.

The reference scatters the mapped labels far-to-near a second time; here `dg_scan_labels` (csrc/label_image.hip) reads the
label of every cell's winner through the z-buffer words the projection left behind, so the label image is the label of the
very record the projected `.npy` holds.  The table is SemanticKITTI's public learning map (semantic-kitti.yaml of the
dataset's API): 34 raw ids onto 20 classes; an id outside it is an error here as it is a KeyError there.
"""
import os

import numpy as np

from .. import _lib as L
from .raw import RawScanError

CLASS_NAMES = ("unlabeled", "car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist", "motorcyclist",
               "road", "parking", "sidewalk", "other-ground", "building", "fence", "vegetation", "trunk", "terrain", "pole",
               "traffic-sign")
NUM_CLASSES = len(CLASS_NAMES)
UNKNOWN = 255   # the table's entry for an id SemanticKITTI does not define

# class -> the raw ids that map onto it (static ids first, then the 25x "moving" twins)
_RAW_IDS = {
    "unlabeled": (0, 1, 52, 99),            # unlabeled, outlier, other-structure, other-object
    "car": (10, 252),
    "bicycle": (11,),
    "motorcycle": (15,),
    "truck": (18, 258),
    "other-vehicle": (13, 16, 20, 256, 257, 259),   # bus, on-rails, other-vehicle and their moving twins
    "person": (30, 254),
    "bicyclist": (31, 253),
    "motorcyclist": (32, 255),
    "road": (40, 60),                       # road, lane-marking
    "parking": (44,),
    "sidewalk": (48,),
    "other-ground": (49,),
    "building": (50,),
    "fence": (51,),
    "vegetation": (70,),
    "trunk": (71,),
    "terrain": (72,),
    "pole": (80,),
    "traffic-sign": (81,),
}


def _build_lut():
    lut = np.full(65536, UNKNOWN, dtype=np.uint8)
    for name, ids in _RAW_IDS.items():
        lut[list(ids)] = CLASS_NAMES.index(name)
    lut.setflags(write=False)
    return lut


SEMANTIC_KITTI_LUT = _build_lut()   # [65536] uint8: entry i = the class of raw id i, 255 = no such id

_palette = None
_dev_luts = {}


def palette():
    """[20,3] uint8 = uint8(cm.turbo(i / 19)[:3] * 255), the reference's palette, from the library's own turbo table (a
    colour map called with a float x reads entry min(int(x * 256), 255))"""
    global _palette
    if _palette is None:
        from ..utils.render import turbo_lut
        table = turbo_lut().numpy().astype(np.float64)
        rows = [min(int(i / (NUM_CLASSES - 1) * 256), 255) for i in range(NUM_CLASSES)]
        # the table holds five-decimal values rounded to float32: round back before the truncating cast
        _palette = np.uint8(np.round(table[rows], 5) * 255)
        _palette.setflags(write=False)
    return _palette


def device_lut(device, lut=None):
    """the table on `device` (SEMANTIC_KITTI_LUT's copy is made once per device)"""
    import torch
    if lut is not None:
        lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1)
        if lut.size != 65536:
            raise ValueError(f"a label table has 65536 entries, got {lut.size}")
        return torch.from_numpy(lut.copy()).to(device)
    key = torch.device(device)
    key = (key.type, key.index if key.index is not None else torch.cuda.current_device())
    if key not in _dev_luts:
        _dev_luts[key] = torch.from_numpy(SEMANTIC_KITTI_LUT.copy()).to(device)
    return _dev_luts[key]


def read_label_file(path, n=None):
    """a SemanticKITTI `.label` file -> [N] uint32 (class id in the lower half, instance id in the upper); n: the number of
    records the scan has"""
    size = os.path.getsize(path)
    if size % 4 or (n is not None and size != 4 * n):
        raise RawScanError([path], f"{size} bytes is not one uint32 label per point" + (f" ({n} points)" if n is not None else ""))
    return np.fromfile(path, dtype=np.uint32)


def launch_scan_labels(keys, offsets, labels, lut, S, H, W, sem, inst, status):
    """dg_scan_labels on device tensors (status is zeroed here)"""
    status.zero_()
    L.check(L.lib().dg_scan_labels(L.ptr(keys), L.ptr(offsets), L.ptr(labels), L.ptr(lut), S, H, W, L.ptr(sem), L.ptr(inst),
                                   L.ptr(status), L.stream_ptr()), "dg_scan_labels")


def unknown_ids(keys, offsets, labels, s, cells, lut=None):
    """the raw ids of scan s's winners that the table does not know (host side: the error path only)"""
    lut = SEMANTIC_KITTI_LUT if lut is None else np.asarray(lut, dtype=np.uint8).reshape(-1)
    k = keys[s * cells:(s + 1) * cells].cpu().numpy().view(np.uint64)
    o = offsets.cpu().numpy()
    win = (k[k != np.uint64(0xFFFFFFFFFFFFFFFF)] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    win = win[win < o[s + 1] - o[s]]
    ids = labels[int(o[s]):int(o[s + 1])].cpu().numpy().view(np.uint32)[win] & 0xFFFF
    return sorted(int(i) for i in np.unique(ids[lut[ids] == UNKNOWN]))


def project_labels(keys, offsets, labels, H, W, names=None, lut=None):
    """the label images of S projected scans.  keys [S*H*W] int64 device tensor as project_scans / project_clouds_beams
    (return_keys=True) left it; offsets [S+1] ints, the projection's; labels [N] uint32 raw SemanticKITTI words in the points'
    order (tensor or array; int32 bit patterns are taken as they are).  -> (sem [S,H,W] uint8 classes, 0 where no point fell,
    inst [S,H,W] int16 tensor holding the uint16 instance ids' bits).  Raises RawScanError, naming the scan (names[s] or its
    index) and the ids, when a winner's id is not in the table - the reference raises a KeyError there."""
    import torch
    assert keys.is_cuda and keys.dtype == torch.int64 and keys.is_contiguous(), (keys.dtype, keys.device)
    dev = keys.device
    o = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
    S, H, W = o.size - 1, int(H), int(W)
    if S < 1 or keys.numel() != S * H * W:
        raise ValueError(f"keys holds {keys.numel()} words, not S H W = {S} x {H} x {W}")
    if torch.is_tensor(labels):
        lab = labels.view(torch.int32) if labels.dtype != torch.int32 else labels
    else:
        lab = torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).reshape(-1).copy())
    lab = lab.reshape(-1).to(dev).contiguous()
    if lab.numel() != int(o[-1]):
        raise ValueError(f"{lab.numel()} labels for {int(o[-1])} points")
    with torch.cuda.device(dev):
        offs = torch.from_numpy(o).to(dev)
        sem = torch.empty(S, H, W, dtype=torch.uint8, device=dev)
        inst = torch.empty(S, H, W, dtype=torch.int16, device=dev)
        status = torch.empty(S, dtype=torch.int32, device=dev)
        if lab.numel() == 0:   # no point, no winner (and no pointer to hand over)
            return sem.zero_(), inst.zero_()
        launch_scan_labels(keys, offs, lab, device_lut(dev, lut), S, H, W, sem, inst, status)
        bad = torch.nonzero(status).flatten().tolist()
    if bad:
        what = [f"{names[s] if names is not None else f'scan {s}'} (ids {unknown_ids(keys, offs, lab, s, H * W, lut)})" for s in bad]
        raise RawScanError(what, "a label id outside the SemanticKITTI table")
    return sem, inst


def write_label_png(path, sem):
    """a class image [H,W] uint8 -> a mode-P PNG with the reference's palette (process_kitti.py:129-131); the file appears
    under its name only when complete"""
    from PIL import Image
    sem = np.ascontiguousarray(sem, dtype=np.uint8)
    assert sem.ndim == 2, sem.shape
    img = Image.frombytes("P", (sem.shape[1], sem.shape[0]), sem.tobytes())
    img.putpalette([int(v) for v in palette().reshape(-1)])
    tmp = path + ".part"
    img.save(tmp, format="PNG")
    os.replace(tmp, path)


def read_label_png(path, return_palette=False):
    """a label PNG -> its class indices [H,W] uint8 (and, with return_palette, its palette bytes [n,3] uint8)"""
    from PIL import Image
    with Image.open(path) as img:
        if img.mode != "P":
            raise ValueError(f"{path}: not a palette image (mode {img.mode})")
        sem = np.array(img, dtype=np.uint8)
        pal = np.array(img.getpalette() or [], dtype=np.uint8).reshape(-1, 3)
    return (sem, pal) if return_palette else sem
