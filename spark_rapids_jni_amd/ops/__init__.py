from . import aggregate, compact, copying, hashing, join, sort  # noqa: F401
