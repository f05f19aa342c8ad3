"""The 2D half of lib/vis.py on the device: the detected skeleton drawn over the frames (gator_amd/csrc/draw2d.hip).

  SkeletonDrawer(skeleton, n_joints, device)   device tensors in, device tensors out; a batch of frames or several people per frame
      .draw(images, joints, ...)                -> [N,H,W,3] uint8 (out=images draws in place)
  vis_2d_keypoints, vis_coco_skeleton           the reference's functions: numpy in, numpy out, one image per call
  rainbow_colors(L)                             the reference's plt.get_cmap('rainbow') colours, without matplotlib

The picture is an ordered, anti-aliased composite of capsules (cv2.line), discs and rings (cv2.circle) with a documented coverage
rule: cov = clamp(extent + 0.5 - distance, 0, 1), quantised to 0..255 and blended in integers, later primitives on top (draw2d.hip's
header comment).  Byte parity with OpenCV's LINE_AA is NOT claimed -- OpenCV's anti-aliasing is a different
fixed-point rule; the documented rule is the contract, as the renderer's lighting model is.  The matplotlib plots of lib/vis.py
(vis_3d_pose) and vis_2d_pose's window and file writing are not part of this package."""
import ctypes

import numpy as np
import torch

from . import _lib

STYLES = {'keypoints': _lib.DRAW_KEYPOINTS, 'coco': _lib.DRAW_COCO}


def rainbow_colors(L):
    """[L,3] float64: matplotlib's 'rainbow' at np.linspace(0, 1, L), reversed to BGR, times 255 (lib/vis.py: vis_2d_keypoints).  The map
    is a 256-entry table of (|2x - 0.5|, sin(pi x), cos(pi x / 2)) clipped to [0, 1], looked up at int(x * 256), 256 taken as 255."""
    x = np.linspace(0, 1, 256)
    lut = np.clip(np.stack([np.abs(2 * x - 0.5), np.sin(x * np.pi), np.cos(x * np.pi / 2)], 1), 0, 1)
    at = np.minimum((np.linspace(0, 1, int(L)) * 256).astype(np.int64), 255)
    return lut[at][:, ::-1] * 255


class SkeletonDrawer(_lib.DeviceHandle):
    PREFIX = 'gator_draw2d'

    def __init__(self, skeleton, n_joints, device='cuda:0'):
        """skeleton: L pairs of joint indices (the reference's kps_line); n_joints: the joints every person has."""
        sk = _lib.host_index(skeleton)
        if sk.ndim != 2 or sk.shape[1] != 2:
            raise ValueError('SkeletonDrawer: skeleton must be [L,2], got %s' % (sk.shape,))
        self.n_limbs, self.n_joints = int(sk.shape[0]), int(n_joints)
        self._skeleton = sk
        self._rainbow = None
        self._create(device, _lib.host_ptr(sk), self.n_limbs, self.n_joints)

    def set_tile_rows(self, rows):
        """Measurement and test hook: 1 or 4 pixel rows a thread in the tile kernel (the same bytes), 0 = the built-in choice."""
        _lib.check(self._lib.gator_draw2d_set_tile_rows(self._h, int(rows)), 'gator_draw2d_set_tile_rows')

    def _colors(self, colors, style):
        if colors is None:
            if style != 'keypoints':
                raise ValueError("draw: style 'coco' needs its colour (vis_coco_skeleton's given_color, on the 0..255 scale)")
            if self._rainbow is None:
                self._rainbow = torch.as_tensor(rainbow_colors(self.n_limbs), dtype=torch.float32).to(self.device)
            return self._rainbow
        c = torch.as_tensor(colors, dtype=torch.float32).to(self.device)
        if c.dim() == 1:
            c = c.reshape(1, 3).expand(self.n_limbs, 3)
        if tuple(c.shape) != (self.n_limbs, 3):
            raise ValueError('draw: colors must be (3,) or [%d,3], got %s' % (self.n_limbs, tuple(c.shape)))
        return c.contiguous()

    def draw(self, images, joints, colors=None, conf=None, bbox=None, image_index=None, kp_thre=0.4, alpha=1.0, style='keypoints', out=None):
        """images [N,H,W,3] uint8 and joints [P,J,2|3] float (x, y[, confidence]; pixels) on the device.  conf [P,J] gives the confidence
        of two-column joints; without either, every joint counts as confident.  colors (3,) or [L,3] in the images' channel order on
        the 0..255 scale (default for 'keypoints': rainbow_colors).  bbox [P,4,2] box corners.  image_index [P] names the frame of each
        person (default: person p in frame p); people of one frame are drawn in person order, later on top.  style 'keypoints'
        (vis_2d_keypoints) or 'coco' (vis_coco_skeleton).  out: a tensor like images, or images itself to draw in place.  -> out."""
        if style not in STYLES:
            raise ValueError("draw: style is 'keypoints' or 'coco', got %r" % (style,))
        _lib.need_device('SkeletonDrawer.draw', images, joints, conf, bbox, out)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous() or images.device != self.device:
            raise ValueError('draw: images must be a contiguous uint8 tensor [N,H,W,3] on %s, got %s %s' % (self.device, images.dtype, tuple(images.shape)))
        if joints.dim() != 3 or joints.shape[1] != self.n_joints or joints.shape[2] not in (2, 3):
            raise ValueError('draw: expected joints [P,%d,2|3], got %s' % (self.n_joints, tuple(joints.shape)))
        j = joints.to(self.device).float()
        if conf is not None:
            if tuple(conf.shape) != tuple(j.shape[:2]):
                raise ValueError('draw: conf must be [P,J] = %s, got %s' % (tuple(j.shape[:2]), tuple(conf.shape)))
            j = torch.cat([j[:, :, :2], conf.to(self.device).float()[:, :, None]], 2)
        j = j.contiguous()
        P, N, H, W = j.shape[0], images.shape[0], images.shape[1], images.shape[2]
        if bbox is not None:
            if tuple(bbox.shape) != (P, 4, 2):
                raise ValueError('draw: bbox must be [P,4,2] corners, got %s' % (tuple(bbox.shape),))
            bbox = bbox.to(self.device).float().contiguous()
        idx = None
        if image_index is not None:
            idx = _lib.host_index(image_index)
            if idx.shape != (P,):
                raise ValueError('draw: image_index must have one entry per person (%d), got %s' % (P, idx.shape))
        if out is None:
            out = torch.empty_like(images)
        elif out.dtype != torch.uint8 or out.shape != images.shape or not out.is_contiguous() or out.device != self.device:
            raise ValueError('draw: out must be a contiguous uint8 tensor like images')
        col = self._colors(colors, style)
        a = _lib.Draw2dArgs(struct_size=ctypes.sizeof(_lib.Draw2dArgs), n_people=P, n_images=N, H=H, W=W, joint_dim=j.shape[2], style=STYLES[style],
                            kp_thre=float(kp_thre), alpha=float(alpha), joints=_lib.ptr(j), colors=_lib.ptr(col), bbox=_lib.ptr(bbox),
                            images=_lib.ptr(images), out=_lib.ptr(out), image_index=_lib.host_ptr(idx))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.gator_draw2d_u8(self._h, ctypes.byref(a), _lib.stream_ptr(self.device)), 'gator_draw2d_u8')
        return out


_DRAWERS = {}


def _drawer(kps_lines, n_joints, device):
    key = (tuple((int(a), int(b)) for a, b in kps_lines), int(n_joints), str(device))
    if key not in _DRAWERS:
        _DRAWERS[key] = SkeletonDrawer(key[0], n_joints, device)
    return _DRAWERS[key]


def _draw_numpy(img, kps, kps_lines, colors, good, bbox, alpha, style, device):
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('expected img as a uint8 array [H,W,3], got %s %s' % (img.dtype, img.shape))
    kps = np.asarray(kps)
    d = _drawer(kps_lines, kps.shape[1], device)
    xy = np.ascontiguousarray(kps[:2].T)
    # the reference converts with astype(np.int32) from the array's own precision: truncate here, before the float32 the device takes
    with np.errstate(invalid='ignore'):
        xy = np.where(np.isfinite(xy), np.clip(np.trunc(xy), -2.0 ** 20, 2.0 ** 20), np.nan).astype(np.float32)
    j = torch.from_numpy(xy[None]).to(d.device)
    conf = None if good is None else torch.from_numpy(np.asarray(good, np.float32)[None]).to(d.device)
    bb = None if bbox is None else torch.from_numpy(np.asarray(bbox, np.float32).reshape(1, 4, 2)).to(d.device)
    c8 = np.clip(np.rint(np.asarray(colors, np.float64)), 0, 255).astype(np.float32)       # rounded where the colour still has its own precision
    frames = torch.from_numpy(img[None]).to(d.device)
    return d.draw(frames, j, colors=c8, conf=conf, bbox=bb, kp_thre=0.5, alpha=alpha, style=style)[0].cpu().numpy()


def vis_2d_keypoints(img, kps, kps_line, bbox=None, kp_thre=0.4, alpha=1, device='cuda:0'):
    """lib/vis.py's vis_2d_keypoints: img [H,W,3] uint8 (BGR), kps [3,J] = (x, y, confidence) rows, kps_line the skeleton's pairs,
    bbox [4,2] corners or None.  -> the image with the skeleton drawn, numpy."""
    kps = np.asarray(kps)
    good = kps[2] > kp_thre          # the reference's comparison, in the array's own precision; the device sees 1 or 0 against 0.5
    return _draw_numpy(img, kps, kps_line, rainbow_colors(len(kps_line)), good, bbox, alpha, 'keypoints', device)


def vis_coco_skeleton(img, kps, kps_lines, given_color, alpha=1, device='cuda:0'):
    """lib/vis.py's vis_coco_skeleton: every limb in given_color (0..1 scale, taken channel for channel as the reference does), no
    confidence test.  kps [2|3,J]."""
    color = [float(given_color[0]) * 255, float(given_color[1]) * 255, float(given_color[2]) * 255]
    return _draw_numpy(img, np.asarray(kps), kps_lines, [color] * len(kps_lines), None, None, alpha, 'coco', device)
