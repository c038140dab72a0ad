"""The data side of the motion generator (stage 1 of the reference pipeline): the training-batch sampler over a dataset written by
parc_amd.util.create_dataset.  The model and the trainer are the reference's own; see INTEGRATION.md for the hand-over."""
