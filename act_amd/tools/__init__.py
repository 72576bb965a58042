from .runner_pretrain import run_net as pretrain_run_net  # noqa: F401
from .runner_autoencoder import run_net as token_run_net  # noqa: F401
from .runner_autoencoder import validate_net as token_val_net  # noqa: F401
from .runner_autoencoder import test_net as token_test_net  # noqa: F401
from .runner_tsne import tsne_net as tsne_run_net  # noqa: F401
