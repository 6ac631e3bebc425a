"""MI355X-native DynaBOA adaptation hot path.

Runtime note: the ROCm runtime multiplexes a process's HIP streams onto a fixed number of hardware queues.  With the reference's
default term set a level runs its chain, the weight-gradient stream and the two pass streams side by side (adapt_step.hip
"par_passes"); when there are fewer queues than streams, streams share a queue and run with less overlap - results are the same.
This package sets no queue count of its own."""
