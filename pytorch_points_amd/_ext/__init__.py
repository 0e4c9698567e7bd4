"""Stand-ins for the reference's pybind modules ``pytorch_points._ext.losses``, ``pytorch_points._ext.sampling``
and ``pytorch_points._ext.linalg`` (same function names and positional signatures), implemented on the C ABI of
libpp_hip.so."""
from . import linalg, losses, sampling  # noqa: F401
