"""Bottom layer of the input chain: the per-device input stream, the pinned staging buffer and the one staged upload
(DESIGN §2.10a).  The LiDAR chain, the GT-sampling paste and the JPEG decode all bring their host data to the device
through ``staged_upload``."""
import torch

_input_streams = {}       # device index -> torch.cuda.Stream for the input chain
_buffers = {}             # device index -> [pinned uint8 buffer, event after its last H2D copy]


def device_index(device):
    """Index of a cuda device; a bare 'cuda' means the current device."""
    return device.index if device.index is not None else torch.cuda.current_device()


def align16(n):
    return (n + 15) // 16 * 16


def input_stream(device):
    """The per-device stream the LiDAR input chain runs on: its H2D copy and passes never queue behind the training
    step on the caller's stream, so the count readback waits for them alone."""
    i = device_index(device)
    s = _input_streams.get(i)
    if s is None:
        s = _input_streams[i] = torch.cuda.Stream(device=torch.device("cuda", i))
    return s


def _buffer(i, nbytes):
    st = _buffers.get(i)
    if st is None or st[0].numel() < nbytes:
        if st is not None:
            st[1].synchronize()
        st = _buffers[i] = [torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        st[1].record(torch.cuda.current_stream(torch.device("cuda", i)))
    else:
        st[1].synchronize()                 # the previous batch's copy out of this buffer has finished
    return st


def staged_upload(device, nbytes, fill, run):
    """One H2D copy of ``nbytes`` host bytes and the work that reads them, off the caller's stream.  The ordering:
      1. the host waits until the previous upload's copy out of the device's pinned buffer has finished (the buffer
         grows when too small), then, with input_stream(device) current, the device buffer ``dev`` is allocated and
         ``fill(host, dev)`` writes the numpy view ``host`` [nbytes]; ``dev`` is there for plans that hold addresses
         inside it (not to be read or written yet);
      2. one asynchronous copy host -> dev on the input stream;
      3. the buffer's ``copied`` event is recorded: the next upload waits on it before it overwrites the buffer;
      4. ``run(dev, stream)`` launches on the input stream and returns a tuple;
      5. a ``done`` event is recorded behind it;
      6. the caller's current stream waits on ``done`` (the host does not);
      7. every tensor of the tuple is handed to the caller's stream (record_stream).  -> run's tuple."""
    i = device_index(device)
    device = torch.device("cuda", i)
    host, copied = _buffer(i, nbytes)
    cur = torch.cuda.current_stream(device)
    s = input_stream(device)
    with torch.cuda.stream(s):
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        fill(host.numpy()[:nbytes], dev)
        dev.copy_(host[:nbytes], non_blocking=True)
        copied.record(s)
        result = run(dev, s)
        done = torch.cuda.Event()
        done.record(s)
    cur.wait_event(done)
    for t in result:
        if torch.is_tensor(t):
            t.record_stream(cur)
    return result
