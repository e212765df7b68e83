"""Post-Newtonian helpers of the frame fixing (scri/pn)."""
from . import boosted_comcharge  # noqa: F401
