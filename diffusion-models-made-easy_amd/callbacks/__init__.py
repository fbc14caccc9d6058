from .generate import GenerateImage  # noqa: F401
