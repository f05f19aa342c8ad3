"""Mirror of the reference's lib/smpl.py `SMPL` wrapper (the datasets' `mesh_model`): the three gendered layers and the tables the
datasets read from it.  It is built from layers handed in -- gator_amd.smpl.SMPLLayer objects made from the caller's own model
files -- instead of `cfg` paths; the H36M / COCO regressors are caller-side files as well and are passed in when wanted."""
import numpy as np

FACE_KPS_VERTEX = (331, 2802, 6262, 3489, 3990)      # nose, L eye, R eye, L ear, R ear as mesh vertices

JOINTS_NAME = ('Pelvis', 'L_Hip', 'R_Hip', 'Torso', 'L_Knee', 'R_Knee', 'Spine', 'L_Ankle', 'R_Ankle', 'Chest', 'L_Toe', 'R_Toe', 'Neck',
               'L_Thorax', 'R_Thorax', 'Head', 'L_Shoulder', 'R_Shoulder', 'L_Elbow', 'R_Elbow', 'L_Wrist', 'R_Wrist', 'L_Hand', 'R_Hand',
               'Nose', 'L_Eye', 'R_Eye', 'L_Ear', 'R_Ear')
FLIP_PAIRS = ((1, 2), (4, 5), (7, 8), (10, 11), (13, 14), (16, 17), (18, 19), (20, 21), (22, 23), (25, 26), (27, 28))
SKELETON = ((0, 1), (1, 4), (4, 7), (7, 10), (0, 2), (2, 5), (5, 8), (8, 11), (0, 3), (3, 6), (6, 9), (9, 14), (14, 17), (17, 19),
            (21, 23), (9, 13), (13, 16), (16, 18), (18, 20), (20, 22), (9, 12), (12, 24), (24, 14), (24, 25), (24, 26), (25, 27), (26, 28))


class SMPL(object):
    def __init__(self, layers, joint_regressor_h36m=None, joint_regressor_coco=None):
        """layers: {'neutral': SMPLLayer[, 'male': ..., 'female': ...]} or one layer (taken as every gender's)."""
        if not isinstance(layers, dict):
            layers = {'male': layers, 'female': layers, 'neutral': layers}
        if 'neutral' not in layers:
            raise ValueError("SMPL: layers needs a 'neutral' entry")
        self.layer = dict(layers)
        neutral = self.layer['neutral']
        self.vertex_num = neutral.num_verts
        self.face = None if neutral.th_faces is None else neutral.th_faces.numpy()
        reg = neutral.th_J_regressor.numpy().astype(np.float32)
        self.face_kps_vertex = FACE_KPS_VERTEX
        if max(FACE_KPS_VERTEX) >= reg.shape[1]:
            raise ValueError('SMPL: the face key points are vertices of the %d-vertex SMPL mesh, the layer has %d' % (6890, reg.shape[1]))
        onehot = np.zeros((len(FACE_KPS_VERTEX), reg.shape[1]), np.float32)
        onehot[np.arange(len(FACE_KPS_VERTEX)), FACE_KPS_VERTEX] = 1.0
        self.joint_regressor = np.concatenate((reg, onehot))
        self.joint_regressor_h36m = None if joint_regressor_h36m is None else np.asarray(joint_regressor_h36m, np.float32)
        self.joint_regressor_coco = None if joint_regressor_coco is None else np.asarray(joint_regressor_coco, np.float32)
        self.joint_num = 29                 # 24 + nose, L/R eye, L/R ear
        self.joints_name = JOINTS_NAME
        self.flip_pairs = FLIP_PAIRS
        self.skeleton = SKELETON
        self.root_joint_idx = self.joints_name.index('Pelvis')

    def get_layer(self, gender):
        return self.layer[gender]
