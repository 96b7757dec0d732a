"""`model: MODSSM` resolves here (utils.get_model looks for class `Name` in module `name`); the model is in mopooled.py, next to MOFM."""
from .mopooled import MODSSM  # noqa: F401
