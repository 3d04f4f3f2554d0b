"""deqsci_amd - MI355X-native DEQ-SCI reconstruction hot path.

The HIP library (lib/libdeqsci_hip.so, C ABI in include/deqsci_hip.h) is loaded lazily by the
first operator call; importing the package never needs a GPU."""
from .operators import A_torch_, At_torch_, initial_point, initial_point_gaptv, phi_sum, LinearOperator, SCIOperator  # noqa: F401
from .gaptv import GAP_TV_rec, denoise_tv_chambolle  # noqa: F401
from .solvers import (EquilibriumProxGradSCI, andersonexp, forward_iteration, DEQFixedPoint,  # noqa: F401
                      EquilibriumADMMSCI, admmexp, DEQFixedPointADMM, initial_point_admm)
from .broyden import broyden, broyden_fixed_point  # noqa: F401
from .epsilon2 import epsilon2  # noqa: F401
from .engine import DEQSCIEngine, sigma_schedule  # noqa: F401
from .networks import FFDNet, DnCNN  # noqa: F401
from .autograd import mse_loss_stats  # noqa: F401
from .optim import DeviceAdam, clip_grad_norm_  # noqa: F401
from .noise import SensorNoise, normal_host, philox4x32_10  # noqa: F401
from .training import (SCITrainingDatasetSubset, TrainStep, TrainingConfig, configure_training, load_mat,  # noqa: F401
                       train_solver_sci)

__version__ = "0.1.0"

# deqsci_amd.synth's names, resolved on first use: the module is also a program (`python -m deqsci_amd.synth write ...`), and runpy
# warns about a module the package has already imported when it starts
_SYNTH_EXPORTS = ("PatchSpec", "SynthTrainLoader", "VideoPool", "load_video", "sample_specs", "synthesize", "write_training_directory")


def __getattr__(name):
    if name in _SYNTH_EXPORTS:
        from . import synth
        return getattr(synth, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
