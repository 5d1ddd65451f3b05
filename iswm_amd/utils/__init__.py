"""Host-side pieces of the hot path that the reference keeps in utils/: the criterion (utils/loss.py) and the input
transforms (utils/ext_transforms.py).  The reference's plotting / scheduler / denormalisation helpers are not on the
training step and are not rebuilt.

The criterion's names are bound on first use: importing utils.ext_transforms (numpy tables and the header's records)
imports neither torch nor the library."""
__all__ = ("CrossEntropyLoss", "FocalLoss", "calculate_class_weights", "calculate_class_weights_resident", "create_loss")


def __getattr__(name):
    if name in __all__:
        from . import loss
        return getattr(loss, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
