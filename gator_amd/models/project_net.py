"""Mirror of the reference's lib/models/project_net.py: the weak-perspective camera layer the demo fits per image
(demo/run.py:123-164,192).  Same class name (spelling included), parameter and forward, so a torch.optim.Adam loop over it runs
as before; fit() replaces that loop with the device fit of gator_amd.camera (one launch for all the steps)."""
import torch
import torch.nn as nn


class OptimzeCamLayer(nn.Module):
    def __init__(self, crop_size):
        super(OptimzeCamLayer, self).__init__()
        self.crop_size = crop_size
        self.img_res = crop_size / 2
        self.cam_param = nn.Parameter(torch.rand((1, 3)))

    def forward(self, pose3d):
        output = pose3d[:, :, :2] + self.cam_param[None, :, 1:]
        output = output * self.cam_param[None, :, :1] * self.img_res + self.img_res
        return output

    def fit(self, joints3d, target, **kw):
        """The demo's loop (demo/run.py:150-157) on the device from the current cam_param: joints3d [1,n,3] (or [n,3]), target
        [1,m,2] in crop pixels; keyword arguments as gator_amd.camera.fit_camera (steps, schedule, n_fit).  Writes the fitted camera
        into cam_param and returns the final mean L1 loss."""
        from .. import camera
        p = joints3d.detach().reshape(1, -1, 3)
        t = target.detach().reshape(1, -1, 2)
        cam, loss = camera.fit_camera(p, t, init=self.cam_param.detach().to(p.device), crop_size=self.crop_size, **kw)
        with torch.no_grad():
            self.cam_param.copy_(cam.to(self.cam_param.device))
        return loss[0]


def get_model(crop_size):
    model = OptimzeCamLayer(crop_size)

    return model
