"""Camera trajectories for the validation videos (the reference's src/visualization/camera_trajectory)."""
