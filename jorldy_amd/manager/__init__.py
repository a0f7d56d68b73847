from .batched_actors import BatchedValueActors, DeviceActorFeed, VecNStepApeX
from .collector import DeviceCollector, NativeCollector, VecCollector

__all__ = ["VecCollector", "NativeCollector", "DeviceCollector","BatchedValueActors", "VecNStepApeX", "DeviceActorFeed"]
