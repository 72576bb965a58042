"""Scatter plot of a t-SNE embedding (reference: utils/tsne_utils.py:337-383, ``plot_tsne``).  The reference's colour tables and its
gene-selection helpers are not carried over: ``plot_tsne`` colours by ``c=y, cmap='Spectral'`` and never reads them."""
import os

import numpy as np


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def plot_tsne(x, y, colors=None, title=None, filename=None, **kwargs):
    """x [N,2] embedding, y [N] labels -> ``filename`` (default ``test.png``), a 5 x 5 inch scatter at 800 dpi coloured by label with the 'Spectral'
    map (``alpha`` 0.8 and ``s`` 25 unless given; ``colors`` is accepted and unused, as in the reference).  Without matplotlib the points go to
    ``<filename>.txt`` instead, one ``x y label`` row per point.  Returns the path written."""
    x, y = _host(x), _host(y)
    filename = "test.png" if filename is None else filename
    print("Number of samples: ", x.shape[0])
    folder = os.path.dirname(filename)
    if folder:
        os.makedirs(folder, exist_ok=True)
    try:
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError:
        path = filename + ".txt"
        np.savetxt(path, np.column_stack([x[:, 0], x[:, 1], y]), fmt=["%.9g", "%.9g", "%d"])
        return path
    fig = Figure(figsize=(5, 5))
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    if title is not None:
        ax.set_title(title)
    ax.scatter(x[:, 0], x[:, 1], c=y, cmap='Spectral', alpha=kwargs.get("alpha", 0.8), s=kwargs.get("s", 25))
    fig.savefig(filename, dpi=800, bbox_inches='tight')
    return filename
