"""`model: MOFM` resolves here (utils.get_model looks for class `Name` in module `name`); the model is in mopooled.py, next to MODSSM."""
from .mopooled import MOFM  # noqa: F401
