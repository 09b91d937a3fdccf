"""Command-line entry points of the package (run as files or imported as scripts.NAME)."""
