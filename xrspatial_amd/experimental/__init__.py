"""Counterpart of `xrspatial.experimental`: polygonize."""
from .polygonize import polygonize  # noqa: F401
