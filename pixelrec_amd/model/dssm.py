"""`model: DSSM` resolves here (utils.get_model looks for class `Name` in module `name`); the model is in pooled.py, next to FM."""
from .pooled import DSSM  # noqa: F401
