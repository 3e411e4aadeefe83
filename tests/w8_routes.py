"""Which C entry point a host module entered.  Every host module of a companion library imports `_on_device` by name from
torchlsq._hip_host and makes each ctypes call into its library through it, so the module's own binding of that name sees exactly the
launches that module makes -- and none of the ops it composes, which live in other modules with bindings of their own."""
import contextlib


@contextlib.contextmanager
def entered(host_module):
    """Within the block `host_module._on_device` appends the C symbol of every function it is given to the yielded list and then
    calls through; the module's binding is put back on exit, also when the block raises."""
    through, names = host_module._on_device, []

    def recording(index, fn, *args):
        names.append(fn.__name__)
        return through(index, fn, *args)

    host_module._on_device = recording
    try:
        yield names
    finally:
        host_module._on_device = through
