"""The yardstick of the 8-bit frame tests: a numpy restatement of the host expressions of `ActiveNeRFMapper.render`
(scripts/pipeline.py:994-1022) and of the viewer (visualization/vis_nerf_habitat.py:142-179) on the float64 stacks that
`render_image_from_pose` returns, followed by the narrowing to 8 bits that `cv2.imwrite` does, read as
sat8 = np.rint (ties to even) of the value clipped to [0, 255], NaN -> 0.  Pure numpy: no GPU, no package import.

Also the inputs that make the precision rules visible: values one float32 step to either side of every k + 0.5 rounding boundary."""
import numpy as np

DEPTH_PIPELINE = (25.0, 1.0, 255.0, 1.0)
DEPTH_VIEWER = (1.0, 10.0, 1.0, 255.0)


def sat8(x):
    """Narrow to uint8: clamp to [0, 255], round to nearest with ties to even, NaN -> 0 (+inf -> 255, -inf -> 0 by the clamp).
    Keeps the precision of `x` (float32 stays float32: the rounding of an exactly representable value does not depend on it)."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.clip(x, 0, 255))
    return np.where(np.isnan(r), 0, r).astype(np.uint8)


def rgb8(rgb):
    """pipeline.py:994: np.float32(rgb_pd * 255) on the float64 stack, then the narrowing."""
    return sat8(np.float32(np.asarray(rgb, np.float64) * 255))


def occ8(acc):
    return sat8(np.asarray(acc, np.float64) * 255)


def dep8(depth, depth_map=DEPTH_PIPELINE):
    """pipeline.py:1003 np.clip(dep * 25, 0, 255) for DEPTH_PIPELINE, the viewer's np.clip(depth / 10, 0, 1) * 255 for DEPTH_VIEWER, and
    np.clip(d * mul / div, 0, hi) * gain for any other (mul, div, hi, gain); all on float64."""
    d = np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore"):
        if tuple(depth_map) == DEPTH_PIPELINE:
            return sat8(np.clip(d * 25, 0, 255))
        if tuple(depth_map) == DEPTH_VIEWER:
            return sat8(np.clip(d / 10, 0, 1) * 255)
        mul, div, hi, gain = depth_map
        return sat8(np.clip(d * mul / div, 0, hi) * gain)


def label_map(sem):
    """pipeline.py:1011: np.argmax over the class axis of the float64 stack (first maximal index; a NaN counts as the maximum)."""
    return np.argmax(np.asarray(sem, np.float64), axis=-1)


def frames(rgb, depth, acc, sem, palette, depth_map=DEPTH_PIPELINE, channel_order="bgr"):
    """All planes of the frames of rgb [...,3], depth [...], acc [...], sem [...,C] with `palette` [K,3] uint8 RGB.  `labels` is int64
    (the caller narrows it when C <= 256)."""
    lab = label_map(sem)
    out = dict(rgb=rgb8(rgb), depth=dep8(depth, depth_map), occ=occ8(acc), sem=np.asarray(palette, np.uint8)[lab], labels=lab)
    if channel_order == "bgr":
        out["rgb"], out["sem"] = out["rgb"][..., ::-1], out["sem"][..., ::-1]       # cv2.cvtColor(..., COLOR_RGB2BGR)
    return out


def depth_f32_form(depth):
    """What a single-precision kernel would compute for the pipeline mapping: the same expression in float32.  NOT the reference."""
    d = np.asarray(depth, np.float32)
    return sat8(np.clip(d * np.float32(25), np.float32(0), np.float32(255)))


def rgb_f64_form(rgb):
    """What a double-precision kernel would compute for the colour plane: no narrowing of the product to float32.  NOT the reference."""
    return sat8(np.asarray(rgb, np.float64) * 255)


def _either_side(centres):
    c = np.asarray(centres, np.float64).astype(np.float32)
    return np.concatenate([np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]).astype(np.float32)


def depth_boundary_set():
    """float32 depths one step above and below (k + 0.5) / 25, k < 255: next to every rounding boundary of clip(d * 25, 0, 255)."""
    return _either_side((np.arange(255) + 0.5) / 25)


def unit_boundary_set():
    """float32 values one step above and below (k + 0.5) / 255, k < 255: next to every rounding boundary of x * 255."""
    return _either_side((np.arange(255) + 0.5) / 255)
