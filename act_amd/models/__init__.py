from .build import build_model_from_cfg, MODELS  # noqa: F401
from . import dvae  # noqa: F401
from . import act  # noqa: F401
from . import bert  # noqa: F401
from . import pointnet2_nets  # noqa: F401
from . import dgcnn_nets  # noqa: F401
from . import pointmlp  # noqa: F401
from . import pct  # noqa: F401
