from . import resnet  # noqa: F401
from . import xception  # noqa: F401  (the reference imports it too; modeling.deeplabv3plus_xception / deeplabv3_xception select it)
