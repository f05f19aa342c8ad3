"""Mirror of the reference's `models` package (lib/models/__init__.py:1-4): `models.GATOR / GAT / MDR / project_net .get_model`."""
from . import GAT, MDR  # noqa: F401  (order matters: GATOR imports both)
from . import project_net  # noqa: F401
from . import GATOR  # noqa: F401
from . import smpl  # noqa: F401  (lib/smpl.py: the SMPL wrapper the datasets hold as mesh_model)
