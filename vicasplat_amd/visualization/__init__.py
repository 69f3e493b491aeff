"""Visualisation of the validation step (the reference's src/visualization): colour maps on the HIP kernels, layout in torch."""
