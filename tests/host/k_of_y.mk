# The host driver of k(y) over many blocks (tests/test_k_of_y_host.py): a plain build and one under the sanitizer flags of the Makefile
# beside it ($(SAN)), which this file includes rather than repeats.
#   make -f k_of_y.mk k_of_y_host k_of_y_host_san
include Makefile
KDEPS = k_of_y_host.cpp $(CSRC)/k_of_y_plan.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp
k_of_y_host: $(KDEPS)
	$(CXX) -O2 -std=c++17 -w k_of_y_host.cpp -o $@
k_of_y_host_san: $(KDEPS)
	$(CXX) $(SAN) k_of_y_host.cpp -o $@
