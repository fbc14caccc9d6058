from .iddpm import cosine_schedule, interpolate_variance, process_coefficients, respaced_coefficients, space_timesteps  # noqa: F401
