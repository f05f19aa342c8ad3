"""The demo's mesh overlay (demo/renderer.py) on the device: a batched software rasteriser (gator_amd/csrc/render.hip).

  MeshRenderer(faces, device)   device tensors in, device tensors out; a batch of frames or several people per frame
      .project(verts, cam)              -> xy_fixed [M,V,2] int32 (24.8 pixels), z [M,V], normals [M,V,3]
      .rasterise(xy_fixed, z, ...)      -> keys [N,H,W] (int64 storage of the uint64 visibility keys)
      .resolve(keys, xy_fixed, normals) -> rgb [N,H,W,3] uint8 (, face_id [N,H,W] int32, depth [N,H,W] f32)
      .render(verts, cam, ...)          -> the three in one call, intermediates kept in the renderer's own workspace
  Renderer(faces, resolution, orig_img, wireframe)   the reference's class: numpy in, numpy out, one image per call

Geometry, visibility and the compositing rule are the reference's (pyrender through a weak-perspective camera).  The LIGHTING is a documented
diffuse model with the reference's scene parameters, lin = base * (ambient + (1/pi) * sum_k I_k * max(0, n . l_k)), out = lin ** (1/2.2):
colour parity with pyrender's shader is not claimed and not measured."""
import math

import numpy as np
import torch

from . import _lib

CULL_BACKFACES = 1                              # include/gator_hip.h: GATOR_RENDER_CULL_BACKFACES
DEMO_AMBIENT = 0.3                              # demo/renderer.py:51
# demo/renderer.py:54-60: two directional lights of intensity 1.2, posed by Rx(-45 deg) and Ry(45 deg); a light shines down its -z, so
# the direction TOWARDS it is +z of its pose, and the model's output coordinates are the scene's with y and z negated (the Rx(180) flip)
DEMO_LIGHTS = ((0.0, -math.sqrt(0.5), -math.sqrt(0.5), 1.2), (math.sqrt(0.5), 0.0, -math.sqrt(0.5), 1.2))
DEMO_COLOR = (1.0, 1.0, 0.9)                    # demo/renderer.py:62


def rotation_matrix(angle_deg, axis):
    """trimesh.transformations.rotation_matrix(radians(angle_deg), axis)[:3, :3] (Rodrigues, the axis normalised), float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(angle_deg)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return math.cos(t) * np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * np.outer(a, a)


def demo_rotation(angle=None, axis=None, rotate=False):
    """The one matrix the reference's render() applies to the flipped mesh (demo/renderer.py:69-79): `rotate` first, then angle/axis."""
    R = np.eye(3)
    if rotate:
        R = rotation_matrix(60.0, [0, 1, 0]) @ R
    if angle and axis:
        R = rotation_matrix(angle, axis) @ R
    return R


class MeshRenderer(_lib.DeviceHandle):
    PREFIX = 'gator_renderer'

    def __init__(self, faces, device='cuda:0', n_verts=None):
        """faces [F,3] integer vertex indices (numpy or tensor); n_verts defaults to the largest index + 1."""
        f = np.ascontiguousarray(np.asarray(faces.cpu() if torch.is_tensor(faces) else faces).astype(np.int64))
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError('MeshRenderer: faces must be [F,3], got %s' % (f.shape,))
        if f.size and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
            raise ValueError('MeshRenderer: a face index does not fit int32')
        self.n_faces = int(f.shape[0])
        self.n_verts = int(n_verts) if n_verts is not None else (int(f.max()) + 1 if f.size else 0)
        self._faces = f.astype(np.int32)
        self._create(device, _lib.host_ptr(self._faces), self.n_faces, self.n_verts)

    def set_small_box(self, pixels):
        _lib.check(self._lib.gator_renderer_set_small_box(self._h, int(pixels)), 'gator_renderer_set_small_box')

    # -- argument plumbing ---------------------------------------------------------------------------------------------------------
    def _meshes(self, verts, cam, who):
        if not verts.is_cuda or not cam.is_cuda:
            raise RuntimeError('%s: verts and cam must live on a HIP device (there is no CPU path)' % who)
        if verts.dim() != 3 or verts.shape[1] != self.n_verts or verts.shape[2] != 3:
            raise ValueError('%s: expected verts [M,%d,3], got %s' % (who, self.n_verts, tuple(verts.shape)))
        if cam.dim() != 2 or cam.shape[1] != 4 or cam.shape[0] != verts.shape[0]:
            raise ValueError('%s: expected cam [M,4] = (sx, sy, tx, ty), got %s' % (who, tuple(cam.shape)))
        return verts.to(self.device).contiguous().float(), cam.to(self.device).contiguous().float()

    def _stage(self, t, dtype, shape, what, who):
        """A stage's device input: on this renderer's device, of the dtype and shape the kernels index by.  -> the contiguous tensor."""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise ValueError('%s: %s must be a %s tensor %s on %s, got %s' % (who, what, dtype, list(shape), self.device,
                                                                             (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t)))
        return t.contiguous()

    @staticmethod
    def _rot(rot):
        if rot is None:
            return None
        r = np.ascontiguousarray(np.asarray(rot, np.float32).reshape(3, 3))
        return r

    @staticmethod
    def _index(image_index, M):
        if image_index is None:
            return None
        idx = _lib.host_index(image_index)
        if idx.shape != (M,):
            raise ValueError('image_index must have one entry per mesh (%d), got %s' % (M, idx.shape))
        return idx

    @staticmethod
    def _lights(lights):
        L = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(-1, 4))
        return L

    def _colors(self, color, M):
        if color is None:
            return None
        c = torch.as_tensor(color, dtype=torch.float32, device=self.device)
        if c.dim() == 1:
            c = c.reshape(1, 3).expand(M, 3)
        if c.shape != (M, 3):
            raise ValueError('color must be (3,) or [M,3], got %s' % (tuple(c.shape),))
        return c.contiguous()

    def _background(self, background, N, H, W):
        if background is None:
            return None
        if not torch.is_tensor(background) or not background.is_cuda or background.dtype != torch.uint8 or tuple(background.shape) != (N, H, W, 3):
            raise ValueError('background must be a uint8 device tensor [%d,%d,%d,3]' % (N, H, W))
        return background.contiguous()

    # -- the three launches --------------------------------------------------------------------------------------------------------
    def project(self, verts, cam, size=(224, 224), rot=None):
        """Stage 1.  size = (W, H).  -> (xy_fixed [M,V,2] int32, z [M,V] f32, normals [M,V,3] f32)."""
        v, c = self._meshes(verts, cam, 'project')
        M, (W, H) = v.shape[0], size
        xy = torch.empty((M, self.n_verts, 2), device=self.device, dtype=torch.int32)
        z = torch.empty((M, self.n_verts), device=self.device, dtype=torch.float32)
        n = torch.empty((M, self.n_verts, 3), device=self.device, dtype=torch.float32)
        r = self._rot(rot)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.gator_render_vertices_f32(self._h, _lib.ptr(v), _lib.ptr(c), M, int(H), int(W), _lib.host_ptr(r),
                                                           _lib.ptr(xy), _lib.ptr(z), _lib.ptr(n), _lib.stream_ptr(self.device)), 'gator_render_vertices_f32')
        return xy, z, n

    def rasterise(self, xy_fixed, z, image_index=None, n_images=None, size=(224, 224), cull_backfaces=True):
        """Stage 2 on stage 1's outputs.  -> keys [N,H,W] int64: the bits of the uint64 keys (depth << 32 | id), -1 where empty."""
        if not torch.is_tensor(xy_fixed) or xy_fixed.dim() != 3:
            raise ValueError('rasterise: xy_fixed must be a tensor [M,%d,2]' % self.n_verts)
        M, (W, H) = xy_fixed.shape[0], size
        xy = self._stage(xy_fixed, torch.int32, (M, self.n_verts, 2), 'xy_fixed', 'rasterise')
        zz = self._stage(z, torch.float32, (M, self.n_verts), 'z', 'rasterise')
        idx = self._index(image_index, M)
        N = int(n_images) if n_images is not None else M
        keys = torch.empty((max(N, 0), max(int(H), 0), max(int(W), 0)), device=self.device, dtype=torch.int64)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.gator_render_raster(self._h, _lib.ptr(xy), _lib.ptr(zz), _lib.host_ptr(idx),
                                                     M, N, int(H), int(W), CULL_BACKFACES if cull_backfaces else 0, _lib.ptr(keys), _lib.stream_ptr(self.device)),
                       'gator_render_raster')
        return keys

    def resolve(self, keys, xy_fixed, normals, background=None, color=DEMO_COLOR, image_index=None, lights=DEMO_LIGHTS, ambient=DEMO_AMBIENT,
                return_face_id=False, return_depth=False):
        """Stage 3.  -> rgb [N,H,W,3] uint8, or (rgb[, face_id][, depth])."""
        if not torch.is_tensor(xy_fixed) or xy_fixed.dim() != 3 or not torch.is_tensor(keys) or keys.dim() != 3:
            raise ValueError('resolve: keys must be a tensor [N,H,W] and xy_fixed a tensor [M,%d,2]' % self.n_verts)
        M = xy_fixed.shape[0]
        N, H, W = keys.shape
        kk = self._stage(keys, torch.int64, (N, H, W), 'keys', 'resolve')
        xy = self._stage(xy_fixed, torch.int32, (M, self.n_verts, 2), 'xy_fixed', 'resolve')
        nn = self._stage(normals, torch.float32, (M, self.n_verts, 3), 'normals', 'resolve')
        idx = self._index(image_index, M)
        col, bg, L = self._colors(color, M), self._background(background, N, H, W), self._lights(lights)
        rgb = torch.empty((N, H, W, 3), device=self.device, dtype=torch.uint8)
        fid = torch.empty((N, H, W), device=self.device, dtype=torch.int32) if return_face_id else None
        dep = torch.empty((N, H, W), device=self.device, dtype=torch.float32) if return_depth else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.gator_render_resolve(self._h, _lib.ptr(kk), _lib.ptr(xy), _lib.ptr(nn), _lib.ptr(col),
                                                      _lib.host_ptr(idx), M, _lib.ptr(bg), N, H, W,
                                                      _lib.host_ptr(L), L.shape[0], float(ambient), _lib.ptr(rgb), _lib.ptr(fid), _lib.ptr(dep),
                                                      _lib.stream_ptr(self.device)), 'gator_render_resolve')
        out = (rgb,) + ((fid,) if return_face_id else ()) + ((dep,) if return_depth else ())
        return out[0] if len(out) == 1 else out

    def render(self, verts, cam, background=None, color=DEMO_COLOR, image_index=None, size=(224, 224), return_face_id=False, return_depth=False,
               n_images=None, rot=None, lights=DEMO_LIGHTS, ambient=DEMO_AMBIENT, cull_backfaces=True):
        """verts [M,V,3], cam [M,4] = (sx, sy, tx, ty) on the device; size = (W, H).  image_index [M] puts several meshes into one image
        (one shared depth buffer); default: mesh m alone in image m.  background [N,H,W,3] uint8 on the device or None (black); color (3,)
        or [M,3], linear.  -> rgb [N,H,W,3] uint8, or (rgb[, face_id [N,H,W] int32, -1 where empty][, depth [N,H,W] f32, +inf where empty])."""
        v, c = self._meshes(verts, cam, 'render')
        M, (W, H) = v.shape[0], (int(size[0]), int(size[1]))
        idx = self._index(image_index, M)
        N = int(n_images) if n_images is not None else (M if background is None else background.shape[0])
        col, bg, L, r = self._colors(color, M), self._background(background, N, H, W), self._lights(lights), self._rot(rot)
        rgb = torch.empty((max(N, 0), max(H, 0), max(W, 0), 3), device=self.device, dtype=torch.uint8)
        fid = torch.empty(rgb.shape[:3], device=self.device, dtype=torch.int32) if return_face_id else None
        dep = torch.empty(rgb.shape[:3], device=self.device, dtype=torch.float32) if return_depth else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.gator_render_f32(self._h, _lib.ptr(v), _lib.ptr(c), _lib.ptr(col), _lib.host_ptr(idx), M,
                                                  _lib.ptr(bg), N, H, W, _lib.host_ptr(r),
                                                  _lib.host_ptr(L), L.shape[0], float(ambient), CULL_BACKFACES if cull_backfaces else 0,
                                                  _lib.ptr(rgb), _lib.ptr(fid), _lib.ptr(dep), _lib.stream_ptr(self.device)), 'gator_render_f32')
        out = (rgb,) + ((fid,) if return_face_id else ()) + ((dep,) if return_depth else ())
        return out[0] if len(out) == 1 else out


def write_obj(path, verts, faces):
    with open(path, 'w') as fh:
        for v in np.asarray(verts, np.float64):
            fh.write('v %.8f %.8f %.8f\n' % tuple(v))
        for f in np.asarray(faces, np.int64):
            fh.write('f %d %d %d\n' % tuple(f + 1))


class Renderer:
    """demo/renderer.py's Renderer: resolution = (viewport width, viewport height); render() takes and returns numpy.  (The demo passes
    (height, width) of its frame as `resolution`, demo/run.py -- a mix-up that only square frames survive; this class keeps the
    constructor's meaning, width first.)"""

    def __init__(self, faces, resolution=(224, 224), orig_img=False, wireframe=False, device='cuda:0'):
        if wireframe:
            raise NotImplementedError('Renderer: wireframe rendering is not part of this package')
        self.resolution = resolution
        self.faces = faces
        self.orig_img = orig_img
        self.wireframe = wireframe
        self.renderer = MeshRenderer(faces, device)

    def render(self, img, verts, cam, angle=None, axis=None, mesh_filename=None, color=(1.0, 1.0, 0.9), rotate=False):
        W, H = int(self.resolution[0]), int(self.resolution[1])
        img = np.asarray(img)
        if img.shape[:2] != (H, W):
            raise ValueError('Renderer.render: img is %s, the viewport is %d x %d (height x width)' % (img.shape, H, W))
        verts = np.asarray(verts, np.float32)
        if mesh_filename is not None:       # the reference exports the flipped (and `rotate`d) mesh, before angle/axis
            flipped = verts.astype(np.float64) * np.array([1.0, -1.0, -1.0])
            write_obj(mesh_filename, flipped @ demo_rotation(rotate=rotate).T, self.faces)
        r = self.renderer
        v = torch.from_numpy(verts).to(r.device)[None]
        c = torch.as_tensor(np.asarray(cam, np.float32).reshape(1, 4), device=r.device)
        rgb, fid = r.render(v, c, color=tuple(color)[:3], size=(W, H), return_face_id=True, rot=demo_rotation(angle, axis, rotate))
        rgb, valid_mask = rgb[0].cpu().numpy(), (fid[0].cpu().numpy() >= 0)[:, :, np.newaxis]
        output_img = rgb * valid_mask + (1 - valid_mask) * img           # demo/renderer.py:108-110
        return output_img.astype(np.uint8)
