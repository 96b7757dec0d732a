"""`model: FM` resolves here (utils.get_model looks for class `Name` in module `name`); the model is in pooled.py, next to DSSM."""
from .pooled import FM  # noqa: F401
