#!/bin/sh
# diagnostic build of the C-ABI library with s_memtime phase stamps (never shipped, never benchmarked)
# the sources are the library's own list (_native.SOURCES)
cd "$(dirname "$0")/../open_knowledge_graph_embeddings_amd/csrc" && \
hipcc -O3 --offload-arch=gfx950 -std=c++17 -DOKGE_STAMPS -shared -fPIC -o ../libokge_hip_stamps.so \
    $(python3 -c "import sys; sys.path.insert(0, '..'); import _native; print(' '.join(_native.SOURCES))")
