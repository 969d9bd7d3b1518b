"""hipGraph capture of launch sequences: the one place that knows the fresh-stream protocol."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch


def capture_graphs(bodies: Sequence[Callable[[], None]], warmup: Optional[Callable[[], None]] = None) -> List:
    """Record each of `bodies` into its own graph, in order, on one fresh stream forked from the current one: the stream
    waits for the current stream, runs `warmup` eagerly (real launches: the caller restores whatever state they step),
    the device is synchronised, the bodies are captured, and the current stream joins."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graphs = []
    with torch.cuda.stream(s):
        if warmup is not None:
            warmup()
        torch.cuda.synchronize()
        for body in bodies:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                body()
            graphs.append(g)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return graphs
