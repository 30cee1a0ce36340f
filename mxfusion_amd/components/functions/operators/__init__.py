from .operators import broadcast_to  # noqa: F401
