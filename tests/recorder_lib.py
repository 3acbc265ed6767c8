"""The call recorder of the Draw tests: put in place of renderer.lib, it lists what a Draw() issues."""


class Recorder:
    """The library with every crychic_* call of its user recorded by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("crychic_"):
            return fn

        def wrapped(*a):
            self.calls.append(name)
            return fn(*a)
        return wrapped
