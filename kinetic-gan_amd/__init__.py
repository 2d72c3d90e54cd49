"""kinetic-gan_amd: MI355X-native st_gcn hot path of Kinetic-GAN."""
from . import graph  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # the training loop's public names, imported on first use (they pull in torch and the native binding)
    if name in ("TrainLoop", "ResidentDataset"):
        from . import train
        return getattr(train, name)
    if name == "Sampler":
        from . import sample
        return sample.Sampler
    raise AttributeError(name)
