"""The shims the reference's dataset loaders end in (src/dataset/shims): augmentation_shim and crop_shim, on the HIP path."""
from .augmentation_shim import apply_augmentation_shim, reflect_extrinsics, reflect_views  # noqa: F401
from .crop_shim import apply_crop_shim, apply_crop_shim_to_views, center_crop, rescale, rescale_and_crop, resample_tables  # noqa: F401
